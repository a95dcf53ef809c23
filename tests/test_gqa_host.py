"""Grouped-query attention without a GPU: the exported symbols, the C-ABI argument checks (returned before any launch, with fake
pointers), the forced-variant rejections that need no device, and the Python shape rule and its helpers."""
import ctypes
import subprocess

import pytest
import torch

from flash_attention_dlrs_amd import _lib, gqa_kv_heads
from flash_attention_dlrs_amd.flash_attention_torch import check_varlen_args, expand_kv, group_sum

GQA_SYMBOLS = ("fa2_fwd_gqa", "fa2_fwd_gqa_variant", "fa2_bwd_gqa", "fa2_bwd_gqa_variant", "fa2_fwd_varlen_gqa",
               "fa2_fwd_varlen_gqa_variant", "fa2_bwd_varlen_gqa", "fa2_bwd_varlen_gqa_variant")
P = 0x10000  # a fake, aligned device address: every call below must return before any launch


def test_symbols_exported_and_declared():
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for s in GQA_SYMBOLS:
        assert s in names, s
        assert s in _lib.SYMBOLS + _lib.BWD_SYMBOLS, s
        assert getattr(_lib.lib(), s).argtypes is not None, s


def _i64(*v):
    return (ctypes.c_int64 * len(v))(*v)


def _dense_strides(B, H, N, d, bnhd=False):
    if bnhd:  # a (B, N, H, d) tensor viewed as (B, H, N, d)
        return (N * H * d, d, H * d, 1)
    return (H * N * d, N * d, d, 1)


def fwd(B=2, H=8, H_kv=2, N=128, d=64, dtype=_lib.FA2_DTYPE_BF16, window=(-1, -1), variant=0, bnhd=False, causal=0):
    qs = _dense_strides(B, H, N, d, bnhd)
    ks = _dense_strides(B, H_kv, N, d, bnhd)
    ls = (H * N, N)
    return _lib.lib().fa2_fwd_gqa_variant(P, P, P, P, P, _i64(*qs), _i64(*ks), _i64(*ks), _i64(*qs), _i64(*ls), B, H, H_kv, N, d,
                                          dtype, causal, 0.125, window[0], window[1], None, variant)


def bwd(B=2, H=8, H_kv=2, N=128, d=64, dtype=_lib.FA2_DTYPE_BF16, window=(-1, -1), variant=0):
    qs = _i64(*_dense_strides(B, H, N, d))
    ks = _i64(*_dense_strides(B, H_kv, N, d))
    return _lib.lib().fa2_bwd_gqa_variant(P, P, P, P, P, P, P, P, P, P, qs, ks, ks, qs, qs, qs, ks, ks, _i64(H * N, N), B, H, H_kv,
                                          N, d, dtype, 0, 0.125, window[0], window[1], None, variant)


def fwd_varlen(H=8, H_kv=2, d=64, window=(-1, -1), variant=0):
    qs, ks = _i64(H * d, d, 1), _i64(H_kv * d, d, 1)
    return _lib.lib().fa2_fwd_varlen_gqa_variant(P, P, P, P, P, qs, ks, ks, qs, 100, P, P, 2, H, H_kv, d, 60, 70, 100, 120,
                                                 _lib.FA2_DTYPE_BF16, 0, 0.125, window[0], window[1], None, variant)


def bwd_varlen(H=8, H_kv=2, d=64, window=(-1, -1), variant=0):
    qs, ks = _i64(H * d, d, 1), _i64(H_kv * d, d, 1)
    return _lib.lib().fa2_bwd_varlen_gqa_variant(P, P, P, P, P, P, P, P, P, P, qs, ks, ks, qs, qs, qs, ks, ks, 100, P, P, 2, H, H_kv,
                                                 d, 60, 70, 100, 120, _lib.FA2_DTYPE_BF16, 0, 0.125, window[0], window[1], None,
                                                 variant)


def _err():
    return _lib.lib().fa2_last_error().decode()


@pytest.mark.parametrize("call", [fwd, bwd, fwd_varlen, bwd_varlen])
@pytest.mark.parametrize("H,H_kv", [(8, 0), (8, -1), (8, 3), (6, 4), (1, 2)])
def test_bad_kv_heads_are_rejected_naming_h_kv(call, H, H_kv):
    assert call(H=H, H_kv=H_kv) == -1
    assert "H_kv" in _err()


@pytest.mark.parametrize("call", [fwd, bwd, fwd_varlen, bwd_varlen])
@pytest.mark.parametrize("window", [(-2, 0), (0, -2), (-5, -5)])
def test_bad_window_side_is_rejected(call, window):
    assert call(window=window) == -1
    assert "window" in _err()


@pytest.mark.parametrize("variant", [_lib.VARIANT_MFMA16, _lib.VARIANT_MFMA16K, _lib.VARIANT_A64, _lib.VARIANT_MFMA32])
def test_non_mergeable_layout_takes_only_the_gqa_forms(variant):
    # a (B, N, H, d) view with B > 1 cannot be merged into an MHA problem: only generic / mfma16d / mfma16d_w4 have GQA forms
    assert fwd(variant=variant, bnhd=True) == -2
    assert "GQA" in _err()


def test_forced_variant_rejections_without_a_device():
    assert bwd(variant=_lib.BWD_VARIANTS["mfma32"]) == -2                 # no GQA form of the fp32 matrix backward
    assert bwd(variant=_lib.BWD_VARIANTS["mfma32"], window=(4, 0)) == -2
    assert fwd_varlen(variant=_lib.VARIANT_A64) == -2                        # varlen: generic, mfma16d, mfma16d_w4 only
    assert fwd_varlen(variant=_lib.VARIANT_MFMA16) == -2
    assert bwd_varlen(variant=_lib.BWD_VARIANTS["mfma32"]) == -2
    assert bwd_varlen(variant=99) == -2


def test_existing_checks_still_apply():
    assert fwd(N=0) == -3
    assert fwd(d=0) == -1
    assert bwd(d=48) == -2                      # the backward wants d = 2^k, as fa2_bwd
    assert fwd(dtype=17) == -2
    assert fwd_varlen(d=0) == -1


# ---- the Python shape rule ----

def _t(*shape):
    return torch.zeros(*shape)


@pytest.mark.parametrize("H,H_kv", [(8, 8), (8, 4), (8, 2), (8, 1), (6, 3), (1, 1)])
def test_shape_rule_accepts_dividing_kv_heads(H, H_kv):
    assert gqa_kv_heads(_t(2, H, 5, 16), _t(2, H_kv, 5, 16), _t(2, H_kv, 5, 16)) == H_kv


@pytest.mark.parametrize("q,k,v", [
    ((2, 8, 5, 16), (2, 3, 5, 16), (2, 3, 5, 16)),    # H % H_kv != 0
    ((2, 4, 5, 16), (2, 8, 5, 16), (2, 8, 5, 16)),    # more KV heads than query heads
    ((2, 8, 5, 16), (2, 2, 6, 16), (2, 2, 6, 16)),    # different N
    ((2, 8, 5, 16), (2, 2, 5, 32), (2, 2, 5, 32)),    # different d
    ((2, 8, 5, 16), (2, 2, 5, 16), (2, 4, 5, 16)),    # K and V differ
    ((2, 8, 5, 16), (1, 2, 5, 16), (1, 2, 5, 16)),    # different B
    ((2, 8, 5, 16), (2, 0, 5, 16), (2, 0, 5, 16)),    # no KV head
    ((8, 5, 16), (2, 5, 16), (2, 5, 16)),             # not 4-D
])
def test_shape_rule_rejects(q, k, v):
    with pytest.raises(ValueError):
        gqa_kv_heads(_t(*q), _t(*k), _t(*v))


def test_varlen_shape_rule_takes_kv_heads():
    cu = torch.tensor([0, 10], dtype=torch.int32)
    Q = torch.zeros(10, 8, 64, dtype=torch.float16)
    for H_kv in (8, 4, 2, 1):
        K = torch.zeros(10, H_kv, 64, dtype=torch.float16)
        check_varlen_args(Q, K, K.clone(), cu, cu, 10, 10, None)
    for K, V in ((torch.zeros(10, 3, 64), torch.zeros(10, 3, 64)), (torch.zeros(10, 2, 64), torch.zeros(10, 4, 64)),
                 (torch.zeros(10, 2, 32), torch.zeros(10, 2, 32))):
        with pytest.raises(ValueError, match="K and V"):
            check_varlen_args(Q, K.half(), V.half(), cu, cu, 10, 10, None)


def test_expand_and_group_sum_are_the_contiguous_grouping():
    K = torch.arange(2 * 3 * 4 * 2, dtype=torch.float64).view(2, 3, 4, 2)
    E = expand_kv(K, 6)
    assert E.shape == (2, 6, 4, 2)
    for h in range(6):
        assert torch.equal(E[:, h], K[:, h // 2])
    assert torch.equal(group_sum(E, 3), 2 * K)
    assert expand_kv(K, 3) is K and group_sum(K, 3) is K
