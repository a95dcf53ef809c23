"""torch surface of the FA-2 forward -- counterpart of the reference's src/flash_attention_torch.py.

Same names, arity, checks, exceptions, padding and return values as the reference:
  MIN_TENSOR_SIZE, convert_triton_dtype           (reference torch.py:5-18)
  FlashAttention, FlashAttentionDeterministic      (reference torch.py:21-158, :161-294)
The forward launches the hand-written gfx950 kernel through the C ABI (include/fa2_fwd.h) instead
of Triton.  `causal` and `scale` are optional extra positional arguments of `.apply` with
reference-preserving defaults (no mask, scale 1).

The backward launches the hand-written gfx950 backward kernels through
include/fa2_bwd.h: D = rowsum(dO * O), then a key-block-owner kernel for dK / dV and a query-block-owner kernel
for dQ -- no cross-workgroup sum, hence deterministic, so FlashAttention and FlashAttentionDeterministic share
it (the reference's two classes differ only in how they serialise the dQ sum, torch.py:86-158 vs :226-294).
"""
import math

import torch

from . import _lib, autotune

MIN_TENSOR_SIZE = 16

_DTYPE_MAP = {
    torch.float64: _lib.FA2_DTYPE_F64,
    torch.float32: _lib.FA2_DTYPE_F32,
    torch.float16: _lib.FA2_DTYPE_F16,
    torch.float8_e5m2: _lib.FA2_DTYPE_F8E5M2,
    # extensions (BASELINE.json configs c3-c5); the reference raises TypeError for these
    torch.bfloat16: _lib.FA2_DTYPE_BF16,
    torch.float8_e4m3fn: _lib.FA2_DTYPE_F8E4M3,
}


def convert_triton_dtype(torch_dtype):
    """torch dtype -> kernel dtype enum (include/fa2_fwd.h FA2_DTYPE_*).  Name kept from the
    reference (torch.py:7-18), where it returns a triton dtype; TypeError for anything unsupported."""
    try:
        return _DTYPE_MAP[torch_dtype]
    except KeyError:
        raise TypeError(f"dtype {torch_dtype} not supported.") from None


def next_power_of_2(n):
    return 1 << (int(n) - 1).bit_length() if n > 1 else 1


def pad_last_dim(t, d_proper):
    """Zero-pad the last dimension to d_proper (reference torch.py:40-45).  fp8 tensors are padded
    through their byte view (0x00 is +0.0 in both fp8 formats)."""
    d = t.shape[-1]
    if d == d_proper:
        return t
    if t.dtype in (torch.float8_e5m2, torch.float8_e4m3fn):
        out = torch.zeros(*t.shape[:-1], d_proper, dtype=torch.uint8, device=t.device)
        out[..., :d] = t.view(torch.uint8)
        return out.view(t.dtype)
    return torch.nn.functional.pad(t, (0, d_proper - d), mode="constant", value=0.0)


def forward_head_size(dtype, B, H, N, d, causal=False):
    """Head size the forward kernels are RUN at.  The kernels take any d (the reference pads every d that is not a power of two,
    torch.py:38-47), but only some on the matrix cores: f16 / bf16 multiples of 8 and fp32 multiples of 4 up to 128.  Everything
    else would run on the VALU kernel, 60-90 times slower than a zero-padded launch (profiles/r03/pad_vs_predicated.jsonl: bf16
    B4 H32 N4096 d = 100: 87.5 ms as it is, 0.98 ms padded to 128, the three pad copies and the slice of O included).  So:
      * f16 / bf16, d not a multiple of 8: pad to 64 (d < 64) or 128 -- the pipelined kernels; as fast as or faster than the next
        multiple of 8 on every shape measured;
      * f16 / bf16, 64 < d < 128 a multiple of 8: the d-predicated kernel as it is on small grids (29 vs 45 us at B2 H8 N1024), padded
        to 128 from 128 Ki rows on (B4 H32 N4096 d = 96: 1.08 -> 0.90 ms); d < 64 a multiple of 8: as it is, except causal problems of
        256 Ki rows and more, which go to the generated d = 64 kernel (+13 .. 26 %, profiles/r03/pad_small_d.jsonl);
      * fp32, d not a multiple of 4: the next multiple of 4 (the predicated fp32 MFMA kernel);
      * fp8, d < 128: 128 (fp8 runs on the matrix cores at that head size only).
    Zero-padding is exact: the extra products are zeros, the extra columns of O are sliced away (torch.py:81-82)."""
    if dtype in (torch.float16, torch.bfloat16) and d <= 128:
        if d % 8:
            return 64 if d < 64 else 128
        if 64 < d < 128 and B * H * N >= 131072:
            return 128
        if d < 64 and causal and B * H * N >= 262144:
            return 64      # (multiples of 8 below 64, causal, large: the generated d = 64 kernel, 0.34 vs 0.43 ms at B4 H32 N4096 d = 16 .. 48;
            #                non-causal the two are level, and below that size the pad copies cost more than they buy)
    if dtype == torch.float32 and d <= 128 and d % 4:
        return (d + 3) // 4 * 4
    if dtype in (torch.float8_e4m3fn, torch.float8_e5m2) and d < 128:
        return 128       # (the fp8 matrix kernels exist at d = 128 only; any other head size would run on the VALU kernel)
    return d


def normalize_window(N, causal, window):
    """Validate and normalise a local-attention window (include/fa2_fwd.h, fa2_fwd_window) -> (causal, window or None).

    window = (left, right), Python ints, -1 = unbounded on that side: key j is visible to query i iff
    i - left <= j <= i + right.  causal also requires j <= i, so right is clamped to 0.  A side >= N - 1 is unbounded; a
    window that then removes nothing beyond plain or causal attention comes back as None (with causal set for the causal
    case), so the caller runs the plain / causal path unchanged.  ValueError for anything but two ints >= -1."""
    if window is None:
        return bool(causal), None
    if not isinstance(window, (tuple, list)) or len(window) != 2:
        raise ValueError(f"window must be a (left, right) pair of ints, got {window!r}")
    for w in window:
        if isinstance(w, bool) or not isinstance(w, int):
            raise ValueError(f"window sides must be Python ints, got {window!r}")
        if w < -1:
            raise ValueError(f"window sides must be >= -1 (-1 = unbounded), got {window!r}")
    full = max(int(N) - 1, 0)
    left, right = (full if (w < 0 or w >= full) else w for w in window)
    if causal:
        right = 0
    if left == full and right == full:
        return bool(causal), None
    if left == full and right == 0:
        return True, None
    return False, (left, right)


def window_head_size(dtype, d):
    """Head size a windowed forward runs at: f16 / bf16 below 128 other than 64 are zero-padded to 64 or 128 (the windowed
    matrix kernel's sizes, like the pad rule of forward_head_size); everything else runs as it is (the VALU kernel)."""
    if dtype in (torch.float16, torch.bfloat16) and d < 128 and d != 64:
        return 64 if d < 64 else 128
    return d


def gqa_kv_heads(Q, K, V):
    """The shape rule of the dense entry points: Q (B, H, N, d), K and V (B, H_kv, N, d) of one shape, H_kv >= 1 dividing H
    (grouped-query attention; H_kv == H is plain multi-head attention, H_kv == 1 multi-query).  Returns H_kv; ValueError for
    anything else.  Pure: takes CPU tensors as well."""
    if Q.dim() != 4 or K.dim() != 4 or V.dim() != 4 or K.shape != V.shape or Q.shape[0] != K.shape[0] \
            or Q.shape[2:] != K.shape[2:] or K.shape[1] < 1:
        raise ValueError(f"Q, K, V must all be of shape (B, H, N, d), K and V (B, H_kv, N, d): got Q {tuple(Q.shape)}, "
                         f"K {tuple(K.shape)}, V {tuple(V.shape)}")
    H, H_kv = Q.shape[1], K.shape[1]
    if H % H_kv != 0:
        raise ValueError(f"the KV heads must divide the query heads: H={H}, H_kv={H_kv}")
    return H_kv


def expand_kv(t, H):
    """K or V (.., H_kv, N, d) expanded to H heads the way GQA groups them (query head h reads KV head h // (H / H_kv)): the
    repeat_interleave a caller needed before fa2_fwd_gqa existed.  For tests and references."""
    return t if t.shape[-3] == H else t.repeat_interleave(H // t.shape[-3], dim=-3)


def group_sum(t, H_kv):
    """dK or dV (.., H, N, d) of expanded K / V summed back over each group of H / H_kv query heads -> (.., H_kv, N, d)."""
    H = t.shape[-3]
    if H == H_kv:
        return t
    return t.unflatten(-3, (H_kv, H // H_kv)).sum(dim=-3)


def _check_inputs(Q, K, V):
    dev = Q.device
    if dev.type != "cuda" or dev != K.device or dev != V.device:
        raise NotImplementedError("Q, K, V must be on the same CUDA device")
    gqa_kv_heads(Q, K, V)
    if Q.dtype != K.dtype or K.dtype != V.dtype:
        raise ValueError("Q, K, V must have same dtype")


def _forward_impl(ctx, Q, K, V, causal, scale, window=None):
    _check_inputs(Q, K, V)
    B, H, N, d = Q.shape
    dtype = convert_triton_dtype(Q.dtype)
    if window is not None:
        causal, window = normalize_window(N, causal, window)
    ctx.window = window
    if window is not None:
        return _forward_window(ctx, Q, K, V, dtype, scale, window)

    # Non-power-of-2 d or d < 16: the reference pads Q, K, V on the host (torch.py:38-47) and returns the O[..., :d] view
    # of a padded O.  The forward kernels take any d (the MFMA kernels zero-fill the missing
    # columns on load, the generic kernel loops to d): head sizes the matrix cores take run as they are, O comes back with
    # exactly d columns; the others are padded as the reference pads them (forward_head_size).  The backward still wants a
    # power of two and pads what it was handed (_backward_impl).
    d_proper = max(next_power_of_2(d), MIN_TENSOR_SIZE)
    padded = d_proper != d
    d_run = forward_head_size(Q.dtype, B, H, N, d, causal)

    # O inherits Q's strides, L is (B, H, N, 1) in the input dtype (reference torch.py:50-51)
    L = torch.empty(B, H, N, 1, dtype=Q.dtype, device=Q.device)
    if d_run != d:
        Qr, Kr, Vr = (pad_last_dim(t, d_run) for t in (Q, K, V))
        Or = torch.empty_like(Qr)
        _lib.fa2_fwd(Qr, Kr, Vr, Or, L, dtype, causal=causal, scale=scale,
                     variant=_pick(Qr, Kr, Vr, Or, L, dtype, causal, scale))
        O = Or[..., :d]        # (a view of the padded O, as the reference returns it: torch.py:81-82)
    else:
        O = torch.empty_like(Q)
        # static gfx950 tile table, or the on-box tuner's choice when FA2_AUTOTUNE=1 (autotune.py; reference:
        # the Triton autotuner keyed on (B, H, N, d), kernels.py:11-15)
        _lib.fa2_fwd(Q, K, V, O, L, dtype, causal=causal, scale=scale,
                     variant=_pick(Q, K, V, O, L, dtype, causal, scale))

    ctx.save_for_backward(Q, K, V, O, L)
    ctx.padded = padded
    ctx.d_used = d_proper
    ctx.d_orig = d
    ctx.causal = bool(causal)
    ctx.scale = float(scale)
    return O


def _pick(Q, K, V, O, L, dtype, causal, scale):
    """The tuner's choice -- except for grouped-query problems, whose K / V heads its key does not see: the static table."""
    if K.shape[1] != Q.shape[1]:
        return _lib.VARIANT_AUTO
    return autotune.pick(Q, K, V, O, L, dtype, causal, scale)


def _forward_window(ctx, Q, K, V, dtype, scale, window):
    """Local attention (normalised window): padded like the plain path where the windowed matrix kernel wants it; the
    autotuner is not consulted (its key does not see the window)."""
    B, H, N, d = Q.shape
    d_proper = max(next_power_of_2(d), MIN_TENSOR_SIZE)
    d_run = window_head_size(Q.dtype, d)
    L = torch.empty(B, H, N, 1, dtype=Q.dtype, device=Q.device)
    if d_run != d:
        Qr, Kr, Vr = (pad_last_dim(t, d_run) for t in (Q, K, V))
        Or = torch.empty_like(Qr)
        _lib.fa2_fwd(Qr, Kr, Vr, Or, L, dtype, causal=False, scale=scale, window=window)
        O = Or[..., :d]
    else:
        O = torch.empty_like(Q)
        _lib.fa2_fwd(Q, K, V, O, L, dtype, causal=False, scale=scale, window=window)
    ctx.save_for_backward(Q, K, V, O, L)
    ctx.padded = d_proper != d
    ctx.d_used = d_proper
    ctx.d_orig = d
    ctx.causal = False
    ctx.scale = float(scale)
    return O


def window_mask(N, causal=False, window=None, device=None):
    """(N, N) boolean mask of the visible (query, key) pairs, or None when nothing is masked (normalize_window)."""
    causal, window = normalize_window(N, causal, window)
    if window is None and not causal:
        return None
    i = torch.arange(N, device=device).view(N, 1)
    j = torch.arange(N, device=device).view(1, N)
    if window is None:
        return j <= i
    return (j >= i - window[0]) & (j <= i + window[1])


def attention_backward_recompute(Q, K, V, O, dO, L, causal=False, scale=1.0, *, window=None):
    """dQ, dK, dV from the saved statistics in plain torch ops: a readable restatement used by the tests only
    (the product path is _backward_native below).
    P = exp2(scale * S * log2e - L) (reference kernels.py:283-285), D = rowsum(dO * O) (kernels.py:120-166).
    window: local attention, as fa2_fwd_window (P is 0 outside the band).  K, V with H_kv < H heads (grouped-query): expanded
    to H heads, dK / dV summed back over each group."""
    f = torch.float64 if Q.dtype == torch.float64 else torch.float32
    H_kv = K.shape[1]
    q, k, v, o, do, l = (t.to(f) for t in (Q, expand_kv(K, Q.shape[1]), expand_kv(V, Q.shape[1]), O, dO, L))
    S = torch.matmul(q, k.transpose(-1, -2)) * (scale * math.log2(math.e))
    if window is not None:
        mask = window_mask(Q.shape[2], causal, window, Q.device)
        if mask is not None:
            S = S.masked_fill(~mask, float("-inf"))
    elif causal:
        N = Q.shape[2]
        mask = torch.ones(N, N, dtype=torch.bool, device=Q.device).tril()
        S = S.masked_fill(~mask, float("-inf"))
    P = torch.exp2(S - l)
    dV = torch.matmul(P.transpose(-1, -2), do)
    dP = torch.matmul(do, v.transpose(-1, -2))
    D = (do * o).sum(dim=-1, keepdim=True)
    dS = P * (dP - D) * scale
    dQ = torch.matmul(dS, k)
    dK = torch.matmul(dS.transpose(-1, -2), q)
    return dQ.to(Q.dtype), group_sum(dK, H_kv).to(K.dtype), group_sum(dV, H_kv).to(V.dtype)


def backward_native(Q, K, V, O, dO, L, causal=False, scale=1.0, variant="auto", *, window=None):
    """Host glue of the backward launch (reference torch.py:101-155): allocate dQ, dK, dV (strides of Q, K, V) and
    the scratch D, launch, return the gradients.  Inputs are already padded to a supported d.  window: local attention
    (normalize_window); a window that reduces to plain or causal attention takes the plain launch.  K, V with H_kv < H heads
    (grouped-query, gqa_kv_heads): dK, dV come back with K's and V's shapes, summed over each group in the kernel."""
    gqa_kv_heads(Q, K, V)
    if window is not None:
        causal, window = normalize_window(Q.shape[2], causal, window)
    dtype = convert_triton_dtype(Q.dtype)
    if Q.dtype in (torch.float8_e5m2, torch.float8_e4m3fn):
        raise TypeError(f"dtype {Q.dtype} not supported by the backward.")
    B, H, N, d = Q.shape
    dQ, dK, dV = torch.empty_like(Q), torch.empty_like(K), torch.empty_like(V)
    # scratch: rowsum(dO * O) and the fp32 row statistic handed from the dQ launch to the dK/dV launch (fa2_bwd.h)
    D = torch.empty(2, B, H, N, 1, dtype=torch.float64 if Q.dtype == torch.float64 else torch.float32, device=Q.device)
    if dO.stride(-1) != 1:
        dO = dO.contiguous()
    _lib.fa2_bwd(Q, K, V, O, dO, L, dQ, dK, dV, D, dtype, causal=causal, scale=scale,
                 variant=_lib.BWD_VARIANTS[variant], window=window)
    return dQ, dK, dV


def _backward_impl(ctx, dO):
    Q, K, V, O, L = ctx.saved_tensors
    if Q.dtype != dO.dtype:
        raise ValueError("dO must have same dtype as inputs")
    if ctx.padded:   # (reference torch.py:91-100 pads in its backward as well)
        Q, K, V, O, dO = (pad_last_dim(t, ctx.d_used) for t in (Q, K, V, O, dO))
    dQ, dK, dV = backward_native(Q, K, V, O, dO, L, ctx.causal, ctx.scale, window=ctx.window)
    if ctx.padded:
        d = ctx.d_orig
        return dQ[..., :d], dK[..., :d], dV[..., :d], None, None, None
    return dQ, dK, dV, None, None, None


class FlashAttention(torch.autograd.Function):
    """O = softmax(Q K^T) V with scale 1 (reference torch.py:21-84).  `FlashAttention.apply(Q, K, V)`;
    optional extras `FlashAttention.apply(Q, K, V, causal, scale, window)`: window = (left, right) is local attention
    (key j visible to query i iff i - left <= j <= i + right, -1 = unbounded; causal clamps right to 0), None the plain call."""

    @staticmethod
    def forward(ctx, Q, K, V, causal=False, scale=1.0, window=None):
        return _forward_impl(ctx, Q, K, V, causal, scale, window)

    @staticmethod
    def backward(ctx, grad_outputs, *args):
        return _backward_impl(ctx, grad_outputs)


class FlashAttentionDeterministic(torch.autograd.Function):
    """Same forward as FlashAttention (the reference's two forwards are identical, torch.py:161-224);
    the recompute backward used here is deterministic by construction.  Same optional extras (causal, scale, window)."""

    @staticmethod
    def forward(ctx, Q, K, V, causal=False, scale=1.0, window=None):
        return _forward_impl(ctx, Q, K, V, causal, scale, window)

    @staticmethod
    def backward(ctx, grad_outputs, *args):
        return _backward_impl(ctx, grad_outputs)


# ---- variable-length (packed) attention: include/fa2_fwd.h fa2_fwd_varlen, include/fa2_bwd.h fa2_bwd_varlen ----

def _seq_bounds(cu, total):
    """Host copy of cu_seqlens -> [(start, end)], clamped exactly as the kernels clamp (fa2_varlen_seq), without max_seqlen."""
    out = []
    c = [min(max(int(x), 0), total) for x in cu.tolist()]
    for b in range(len(c) - 1):
        out.append((c[b], max(c[b + 1], c[b])))
    return out


def varlen_mask(cu_seqlens_q, cu_seqlens_k, causal=False, window=None, total_q=None, total_k=None):
    """(total_q, total_k) boolean mask of the visible (query token, key token) pairs of a packed batch: block-diagonal over the
    sequences, bottom-right aligned inside each -- query i of a sequence of N_q queries and N_k keys sees key j iff
    i + (N_k - N_q) - left <= j <= i + (N_k - N_q) + right, with -1 unbounded and causal clamping right to 0 (fa2_fwd_varlen).
    For tests and docs; built on the CPU."""
    cq, ck = cu_seqlens_q.cpu(), cu_seqlens_k.cpu()
    total_q = int(cq[-1]) if total_q is None else total_q
    total_k = int(ck[-1]) if total_k is None else total_k
    left, right = (-1, -1) if window is None else window
    mask = torch.zeros(total_q, total_k, dtype=torch.bool)
    for (q0, q1), (k0, k1) in zip(_seq_bounds(cq, total_q), _seq_bounds(ck, total_k)):
        nq, nk = q1 - q0, k1 - k0
        if nq == 0 or nk == 0:
            continue
        i = torch.arange(nq).view(nq, 1) + (nk - nq)
        j = torch.arange(nk).view(1, nk)
        m = torch.ones(nq, nk, dtype=torch.bool)
        if left >= 0:
            m &= j >= i - left
        r = 0 if causal else right
        if r >= 0:
            m &= j <= i + r
        mask[q0:q1, k0:k1] = m
    return mask


def check_varlen_args(Q, K, V, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, window):
    """ValueError for what the varlen entry points cannot take (shapes, dtypes, offsets, window); the CUDA-device check is
    _check_varlen_device's."""
    dev = Q.device
    if Q.dim() != 3 or K.dim() != 3 or V.dim() != 3:
        raise ValueError(f"varlen: Q, K, V must be (total, H, d), got {tuple(Q.shape)}, {tuple(K.shape)}, {tuple(V.shape)}")
    if K.shape != V.shape or Q.shape[2] != K.shape[2] or K.shape[1] < 1 or Q.shape[1] % K.shape[1] != 0:
        raise ValueError(f"varlen: K and V must be (total_k, H, d) with Q's H and d, or (total_k, H_kv, d) with H_kv dividing "
                         f"Q's H, got Q {tuple(Q.shape)}, K {tuple(K.shape)}, V {tuple(V.shape)}")
    if Q.dtype != K.dtype or K.dtype != V.dtype:
        raise ValueError("varlen: Q, K, V must have the same dtype")
    if Q.dtype in (torch.float8_e5m2, torch.float8_e4m3fn):
        raise ValueError(f"varlen: dtype {Q.dtype} is not supported (no backward; e4m3fn cannot hold L = +inf)")
    convert_triton_dtype(Q.dtype)
    for name, cu in (("cu_seqlens_q", cu_seqlens_q), ("cu_seqlens_k", cu_seqlens_k)):
        if not isinstance(cu, torch.Tensor) or cu.dtype != torch.int32 or cu.dim() != 1 or not cu.is_contiguous():
            raise ValueError(f"varlen: {name} must be a contiguous 1-D int32 tensor")
        if cu.device != dev:
            raise ValueError(f"varlen: {name} must be on Q's device ({dev}), got {cu.device}")
        if cu.numel() < 2:
            raise ValueError(f"varlen: {name} must have B + 1 >= 2 entries, got {cu.numel()}")
    if cu_seqlens_q.numel() != cu_seqlens_k.numel():
        raise ValueError(f"varlen: cu_seqlens_q and cu_seqlens_k must both have B + 1 entries, got {cu_seqlens_q.numel()} "
                         f"and {cu_seqlens_k.numel()}")
    for name, m in (("max_seqlen_q", max_seqlen_q), ("max_seqlen_k", max_seqlen_k)):
        if isinstance(m, bool) or not isinstance(m, int) or m < 0:
            raise ValueError(f"varlen: {name} must be an int >= 0, got {m!r}")
    if window is not None:
        normalize_window(1, False, window)  # the sides' own rules (pair of ints >= -1); the shift is per sequence


def _check_varlen_device(Q, K, V):
    dev = Q.device
    if dev.type != "cuda" or dev != K.device or dev != V.device:
        raise NotImplementedError("Q, K, V must be on the same CUDA device")


def varlen_head_size(dtype, d, backward=False):
    """Head size a varlen launch runs at: the forward pads like window_head_size, the backward to a power of two >= 16."""
    if backward:
        return max(next_power_of_2(d), MIN_TENSOR_SIZE)
    return window_head_size(dtype, d)


def varlen_forward(Q, K, V, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, *, causal=False, scale=1.0, window=None,
                   variant="auto"):
    """(O, L) of a packed batch: O (total_q, H, d) contiguous, L (H, total_q) in the I/O dtype.  A forced variant gets the
    tensors as they are; auto pads the head size for the matrix kernel (varlen_head_size)."""
    _check_varlen_device(Q, K, V)
    check_varlen_args(Q, K, V, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, window)
    total_q, H, d_out = Q.shape
    d = varlen_head_size(Q.dtype, d_out) if variant == "auto" else d_out
    if d != d_out:
        Q, K, V = (pad_last_dim(t, d) for t in (Q, K, V))
    O = torch.empty(total_q, H, d, dtype=Q.dtype, device=Q.device)
    L = torch.empty(H, total_q, dtype=Q.dtype, device=Q.device)
    _lib.fa2_fwd_varlen(Q, K, V, O, L, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, convert_triton_dtype(Q.dtype),
                        causal=causal, scale=scale, window=window, variant=_lib.VARIANTS[variant])
    if d != d_out:
        O = O[..., :d_out].contiguous()
    return O, L


def check_varlen_dv_args(Q, K, V, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, window):
    """check_varlen_args with the V rule relaxed for a value head size of its own (fa2_fwd_varlen_dv): V.shape[:2] == K.shape[:2],
    any last axis in [1, 512]."""
    if Q.dim() != 3 or K.dim() != 3 or V.dim() != 3:
        raise ValueError(f"varlen: Q, K, V must be (total, H, d), got {tuple(Q.shape)}, {tuple(K.shape)}, {tuple(V.shape)}")
    if V.shape[:2] != K.shape[:2] or not 1 <= V.shape[2] <= 512:
        raise ValueError(f"varlen: V must be (total_k, H_kv, d_v) with K's total_k and H_kv and d_v in [1, 512], got "
                         f"K {tuple(K.shape)}, V {tuple(V.shape)}")
    check_varlen_args(Q, K, K, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, window)  # (every rule but V's shape)
    if V.dtype != K.dtype:
        raise ValueError("varlen: Q, K, V must have the same dtype")


def mla_prefill_forward(Q, K, V, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, *, causal=False, scale=1.0, window=None,
                        variant="auto"):
    """(O, L) of a packed batch with a value head size of its own (fa2_fwd_varlen_dv; un-absorbed MLA prefill at d 192 / d_v 128):
    O (total_q, H, d_v) contiguous, L (H, total_q) in the I/O dtype.  The tensors go to the library as they are, strides included:
    no head-size padding under any variant."""
    _check_varlen_device(Q, K, V)
    check_varlen_dv_args(Q, K, V, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, window)
    if variant not in _lib.VARLEN_DV_VARIANTS:
        raise ValueError(f"mla prefill: variant must be one of {sorted(_lib.VARLEN_DV_VARIANTS)}, got {variant!r}")
    total_q, H, _ = Q.shape
    O = torch.empty(total_q, H, V.shape[2], dtype=Q.dtype, device=Q.device)
    L = torch.empty(H, total_q, dtype=Q.dtype, device=Q.device)
    _lib.fa2_fwd_varlen_dv(Q, K, V, O, L, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, convert_triton_dtype(Q.dtype),
                           causal=causal, scale=scale, window=window, variant=_lib.VARLEN_DV_VARIANTS[variant])
    return O, L


def mla_prefill_backward(Q, K, V, O, dO, L, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, *, causal=False, scale=1.0,
                         window=None, variant="auto"):
    """(dQ, dK, dV) of mla_prefill_forward from its O and L (fa2_bwd_varlen_dv), with Q's, K's and V's shapes: the matrix kernel for
    f16 / bf16 at d 192 / d_v 128 under "auto", else the VALU kernel at the head sizes given.  The tensors go to the library as they
    are, strides included: no head-size padding under any variant.  Tokens outside every sequence are not written."""
    check_varlen_dv_args(Q, K, V, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, window)
    if variant not in _lib.BWD_VARLEN_DV_VARIANTS:
        raise ValueError(f"mla prefill backward: variant must be one of {sorted(_lib.BWD_VARLEN_DV_VARIANTS)}, got {variant!r}")
    total_q, H, _ = Q.shape
    o_shape = (total_q, H, V.shape[2])
    if tuple(O.shape) != o_shape or tuple(dO.shape) != o_shape or O.dtype != Q.dtype or dO.dtype != Q.dtype:
        raise ValueError(f"mla prefill backward: O and dO must be {o_shape} in Q's dtype, got {tuple(O.shape)} {O.dtype} and "
                         f"{tuple(dO.shape)} {dO.dtype}")
    if tuple(L.shape) != (H, total_q) or L.dtype != Q.dtype or L.stride(1) != 1:
        raise ValueError(f"mla prefill backward: L must be ({H}, {total_q}) in Q's dtype with unit token stride")
    _check_varlen_device(Q, K, V)
    dQ, dK, dV = torch.empty_like(Q), torch.empty_like(K), torch.empty_like(V)
    D = torch.empty(2, H, total_q, dtype=torch.float64 if Q.dtype == torch.float64 else torch.float32, device=Q.device)
    _lib.fa2_bwd_varlen_dv(Q, K, V, O, dO, L, dQ, dK, dV, D, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k,
                           convert_triton_dtype(Q.dtype), causal=causal, scale=scale, window=window,
                           variant=_lib.BWD_VARLEN_DV_VARIANTS[variant])
    return dQ, dK, dV


class FlashAttentionMLAPrefill(torch.autograd.Function):
    """Packed attention with a value head size of its own (un-absorbed MLA prefill, d 192 / d_v 128):
    `FlashAttentionMLAPrefill.apply(Q, K, V, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, causal, scale, window)`,
    Q (total_q, H, d), K (total_k, H_kv, d), V (total_k, H_kv, d_v) with H_kv dividing H, FlashAttentionVarlen's masks and
    conventions.  Returns O (total_q, H, d_v); the cu_seqlens and the other arguments get no gradient.  K may be the broadcast of a
    shared rotary head (`expand`): autograd sums its gradient."""

    @staticmethod
    def forward(ctx, Q, K, V, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, causal=False, scale=1.0, window=None):
        O, L = mla_prefill_forward(Q, K, V, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, causal=causal, scale=scale,
                                   window=window)
        ctx.save_for_backward(Q, K, V, O, L, cu_seqlens_q, cu_seqlens_k)
        ctx.args = (max_seqlen_q, max_seqlen_k, bool(causal), float(scale), window)
        ctx.mark_non_differentiable(L)
        return O

    @staticmethod
    def backward(ctx, dO, *args):
        Q, K, V, O, L, cu_q, cu_k = ctx.saved_tensors
        max_q, max_k, causal, scale, window = ctx.args
        if dO.stride(-1) != 1:
            dO = dO.contiguous()
        dQ, dK, dV = mla_prefill_backward(Q, K, V, O, dO, L, cu_q, cu_k, max_q, max_k, causal=causal, scale=scale, window=window)
        return dQ, dK, dV, None, None, None, None, None, None, None


def varlen_backward(Q, K, V, O, dO, L, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, *, causal=False, scale=1.0,
                    window=None, variant="auto"):
    """(dQ, dK, dV) of a packed batch from the forward's O and L (fa2_bwd_varlen): the MFMA kernel for f16 / bf16 at
    d = 64 / 128 under AUTO, else the VALU kernel, d padded to a power of two >= 16.  Tokens outside every sequence are not
    written (include/fa2_bwd.h)."""
    _check_varlen_device(Q, K, V)
    check_varlen_args(Q, K, V, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, window)
    if O.shape != Q.shape or dO.shape != Q.shape or O.dtype != Q.dtype or dO.dtype != Q.dtype:
        raise ValueError("varlen backward: O and dO must have Q's shape and dtype")
    total_q, H, d = Q.shape
    if L.shape != (H, total_q) or L.dtype != Q.dtype or L.stride(1) != 1:
        raise ValueError(f"varlen backward: L must be ({H}, {total_q}) in Q's dtype with unit token stride")
    d_pow = varlen_head_size(Q.dtype, d, backward=True)
    if d_pow != d:
        Q, K, V, O, dO = (pad_last_dim(t, d_pow) for t in (Q, K, V, O, dO))
    dQ, dK, dV = torch.empty_like(Q), torch.empty_like(K), torch.empty_like(V)
    D = torch.empty(2, H, total_q, dtype=torch.float64 if Q.dtype == torch.float64 else torch.float32, device=Q.device)
    _lib.fa2_bwd_varlen(Q, K, V, O, dO, L, dQ, dK, dV, D, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k,
                        convert_triton_dtype(Q.dtype), causal=causal, scale=scale, window=window,
                        variant=_lib.BWD_VARIANTS[variant])
    if d_pow != d:
        return dQ[..., :d], dK[..., :d], dV[..., :d]
    return dQ, dK, dV


class FlashAttentionVarlen(torch.autograd.Function):
    """Packed variable-length attention (flash_attn_varlen_func's calling convention):
    `FlashAttentionVarlen.apply(Q, K, V, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, causal, scale, window)`,
    Q (total_q, H, d), K / V (total_k, H, d) or (total_k, H_kv, d) with H_kv dividing H (grouped-query), bottom-right aligned
    causal mask and window (include/fa2_fwd.h).  Returns O; the cu_seqlens and the other arguments get no gradient.  Tokens outside every sequence (cu_seqlens[-1] < total, or gaps
    between sequences) are left unwritten in O and in the gradients, as flash-attn leaves them: such a batch must not feed
    them on."""

    @staticmethod
    def forward(ctx, Q, K, V, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, causal=False, scale=1.0, window=None):
        O, L = varlen_forward(Q, K, V, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, causal=causal, scale=scale,
                              window=window)
        ctx.save_for_backward(Q, K, V, O, L, cu_seqlens_q, cu_seqlens_k)
        ctx.args = (max_seqlen_q, max_seqlen_k, bool(causal), float(scale), window)
        ctx.mark_non_differentiable(L)
        return O

    @staticmethod
    def backward(ctx, dO, *args):
        Q, K, V, O, L, cu_q, cu_k = ctx.saved_tensors
        max_q, max_k, causal, scale, window = ctx.args
        if dO.stride(-1) != 1:
            dO = dO.contiguous()
        dQ, dK, dV = varlen_backward(Q, K, V, O, dO, L, cu_q, cu_k, max_q, max_k, causal=causal, scale=scale, window=window)
        return dQ, dK, dV, None, None, None, None, None, None, None
