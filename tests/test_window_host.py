"""Local (sliding-window) attention, host side: the window normalisation, argument errors before any launch, the exported
symbols, the fp64 windowed reference the GPU tests use, and the sharded pass-through.  No GPU."""
import ctypes
import math
import subprocess

import pytest
import torch

from flash_attention_dlrs_amd import _lib, sharded
from flash_attention_dlrs_amd.flash_attention_torch import normalize_window, window_mask


def window_reference(Q, K, V, causal=False, scale=1.0, window=None):
    """fp64 truth: O = softmax(scale Q K^T over the visible keys) V and L = log2-sum-exp2 of scale log2(e) Q K^T over them"""
    q, k, v = (t.double() for t in (Q, K, V))
    S = torch.matmul(q, k.transpose(-1, -2)) * scale
    mask = window_mask(Q.shape[2], causal, window, Q.device)
    if mask is not None:
        S = S.masked_fill(~mask, float("-inf"))
    O = torch.matmul(torch.softmax(S, dim=-1), v)
    L = torch.logsumexp(S, dim=-1, keepdim=True) * math.log2(math.e)
    return O, L


# ---- normalisation (the C layer applies the same rules: fa2_window_normalise)

@pytest.mark.parametrize("N,causal,window,expect", [
    (100, False, None, (False, None)),
    (100, True, None, (True, None)),
    (100, False, (-1, -1), (False, None)),
    (100, False, (99, 99), (False, None)),          # sides >= N - 1 remove nothing
    (100, False, (500, -1), (False, None)),
    (100, False, (-1, 0), (True, None)),            # = causal
    (100, True, (-1, 5), (True, None)),             # causal clamps right to 0
    (100, True, (-1, -1), (True, None)),
    (100, True, (99, 3), (True, None)),
    (100, False, (10, 0), (False, (10, 0))),
    (100, True, (10, 7), (False, (10, 0))),         # causal folded into the window
    (100, False, (0, 0), (False, (0, 0))),
    (100, False, (-1, 300), (False, None)),
    (100, False, (-1, 30), (False, (99, 30))),      # the unbounded side becomes N - 1
    (100, False, (30, 98), (False, (30, 98))),
    (1, False, (0, 0), (False, None)),              # N = 1: nothing can be masked
    (1, True, (0, 0), (True, None)),
])
def test_normalize_window(N, causal, window, expect):
    assert normalize_window(N, causal, window) == expect


@pytest.mark.parametrize("window", [(-2, 0), (0, -5), (1.0, 2), (1, "2"), (True, 1), (1,), (1, 2, 3), 5, "ab"])
def test_normalize_window_rejects(window):
    with pytest.raises(ValueError):
        normalize_window(64, False, window)


def test_window_mask_matches_definition():
    N = 37
    for causal, window in ((False, (3, 5)), (True, (4, 9)), (False, (0, 0)), (False, (-1, 2)), (True, None)):
        m = window_mask(N, causal, window)
        left, right = window if window is not None else (-1, -1)
        for i in range(N):
            for j in range(N):
                vis = (left < 0 or j >= i - left) and (right < 0 or j <= i + right) and (not causal or j <= i)
                assert bool(m[i, j]) == vis, (causal, window, i, j)
    assert window_mask(N, False, (-1, -1)) is None


# ---- the C ABI: argument errors before any launch

def _fwd_window(wl, wr, N=64, d=64, ptr=0x1000, dtype=_lib.FA2_DTYPE_F32):
    s = (N * d, N * d, d, 1)
    i64 = lambda v: (ctypes.c_int64 * len(v))(*v)
    return _lib.lib().fa2_fwd_window(ptr, ptr, ptr, ptr, ptr, i64(s), i64(s), i64(s), i64(s), i64((N, N)),
                                     1, 1, N, d, dtype, 0, 1.0, wl, wr, None)


def _bwd_window(wl, wr, N=64, d=64, ptr=0x1000):
    s = (N * d, N * d, d, 1)
    i64 = lambda v: (ctypes.c_int64 * len(v))(*v)
    st = [i64(s) for _ in range(8)]
    return _lib.lib().fa2_bwd_window(ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, *st, i64((N, N)),
                                     1, 1, N, d, _lib.FA2_DTYPE_F32, 0, 1.0, wl, wr, None)


@pytest.mark.parametrize("wl,wr", [(-2, 0), (0, -2), (-7, -7)])
def test_window_abi_rejects_bad_sides(wl, wr):
    assert _fwd_window(wl, wr) == -1
    assert "window" in _lib.lib().fa2_last_error().decode()
    assert _bwd_window(wl, wr) == -1
    assert "window" in _lib.lib().fa2_last_error().decode()


def test_window_abi_validates_like_the_plain_call():
    assert _fwd_window(3, 0, ptr=0) == -1
    assert "null" in _lib.lib().fa2_last_error().decode()
    assert _fwd_window(3, 0, N=0) == -3


def test_window_forced_variant_without_a_window_form_is_unsupported():
    N, d = 64, 128
    s = (N * d, N * d, d, 1)
    i64 = lambda v: (ctypes.c_int64 * len(v))(*v)
    rc = _lib.lib().fa2_fwd_window_variant(0x1000, 0x1000, 0x1000, 0x1000, 0x1000, i64(s), i64(s), i64(s), i64(s), i64((N, N)),
                                           1, 1, N, d, _lib.FA2_DTYPE_BF16, 0, 1.0, 8, 0, None, _lib.VARIANT_A64)
    assert rc == -2 and "window" in _lib.lib().fa2_last_error().decode()


def test_window_symbols_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    for name in ("fa2_fwd_window", "fa2_fwd_window_variant", "fa2_bwd_window", "fa2_bwd_window_variant"):
        assert f" T {name}\n" in out, name
        assert name in _lib.SYMBOLS + _lib.BWD_SYMBOLS


# ---- the reference the GPU tests use, pinned against torch SDPA

@pytest.mark.parametrize("N,causal,window", [(50, False, (3, 5)), (50, True, (7, 0)), (64, False, (0, 0)), (33, False, (-1, 4)),
                                             (40, True, (10, 10))])
def test_window_reference_matches_sdpa_with_mask(N, causal, window):
    torch.manual_seed(N)
    Q, K, V = (torch.randn(2, 3, N, 16, dtype=torch.float64) for _ in range(3))
    O, L = window_reference(Q, K, V, causal, 0.3, window)
    mask = window_mask(N, causal, window)
    O_sdpa = torch.nn.functional.scaled_dot_product_attention(Q, K, V, attn_mask=mask, scale=0.3)
    assert torch.allclose(O, O_sdpa, atol=1e-12, rtol=0)
    assert torch.isfinite(L).all()


def test_window_reference_causal_equals_causal_sdpa():
    torch.manual_seed(1)
    Q, K, V = (torch.randn(1, 2, 45, 16, dtype=torch.float64) for _ in range(3))
    O, _ = window_reference(Q, K, V, False, 1.0, (-1, 0))
    O_sdpa = torch.nn.functional.scaled_dot_product_attention(Q, K, V, is_causal=True, scale=1.0)
    assert torch.allclose(O, O_sdpa, atol=1e-12, rtol=0)


# ---- sharding

def test_sharded_forward_passes_the_window_to_its_local_forward():
    seen = []

    def local_forward(Q, K, V, causal, scale, window=None):
        seen.append(window)
        return window_reference(Q, K, V, causal, scale, window)

    Q, K, V = (torch.randn(1, 2, 20, 8, dtype=torch.float64) for _ in range(3))
    O, L = sharded.flash_attention_forward_sharded(Q, K, V, causal=True, window=(4, 0), gather=False,
                                                   local_forward=local_forward)
    assert seen == [(4, 0)]
    assert torch.equal(O, window_reference(Q, K, V, True, 1.0, (4, 0))[0])

    def five_args(Q, K, V, causal, scale):  # no window: called exactly as before
        seen.append("five")
        return window_reference(Q, K, V, causal, scale)

    sharded.flash_attention_forward_sharded(Q, K, V, gather=False, local_forward=five_args)
    assert seen[-1] == "five"


def test_sharded_backward_passes_the_window():
    seen = []

    def local_backward(Q, K, V, O, dO, L, causal, scale, window=None):
        seen.append(window)
        return Q, K, V

    t = torch.zeros(1, 1, 4, 8)
    sharded.flash_attention_backward_sharded(t, t, t, t, t, t, window=(2, 2), local_backward=local_backward)
    sharded.flash_attention_backward_sharded(t, t, t, t, t, t, local_backward=lambda *a: seen.append(len(a)) or a[:3])
    assert seen == [(2, 2), 8]
