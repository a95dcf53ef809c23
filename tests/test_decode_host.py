"""KV-cache decode attention (fa2_fwd_kvcache), the part that needs no GPU: the exported symbols, every argument error before any
launch (fake pointers), the workspace size, the split heuristic, the Python wrapper's shape errors, and the arithmetic of the
combine step restated in numpy against the unsplit softmax."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT

import flash_attention_dlrs_amd as fa
from flash_attention_dlrs_amd import _lib

NEW = ("fa2_fwd_kvcache", "fa2_fwd_kvcache_variant", "fa2_kvcache_workspace_bytes", "fa2_kvcache_num_splits")
KEY_TILE = 64


def test_symbols_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "fa2_fwd.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    for name in NEW:
        assert name in _lib.SYMBOLS
        assert re.search(rf"\b{name}\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)), name
        assert re.search(rf"\bT {name}\b", out), name
    for macro, value in (("FA2_KVCACHE_VARIANT_AUTO", 0), ("FA2_KVCACHE_VARIANT_GENERIC", 1), ("FA2_KVCACHE_VARIANT_MFMA16", 2),
                         ("FA2_KVCACHE_MAX_SPLITS", 128)):
        assert re.search(rf"#define {macro} {value}\b", header), macro
    assert _lib.KVCACHE_VARIANTS == {"auto": 0, "generic": 1, "mfma16": 2}
    assert "kvcache" not in " ".join(_lib.VARIANTS)  # decode has its own enum


def _call(ptr=0x1000, null=None, B=2, H=8, H_kv=2, N_q=1, S_k=512, d=64, dtype=_lib.FA2_DTYPE_BF16, window=(-1, -1), num_splits=1,
          ws=None, ws_bytes=0, variant=0, q_strides=None, k_strides=None, l_strides=None, scale=1.0):
    i64 = lambda v: (ctypes.c_int64 * len(v))(*v)
    qs = q_strides or (H * N_q * d, N_q * d, d, 1)
    ks = k_strides or (H_kv * S_k * d, S_k * d, d, 1)
    ls = l_strides or (H * N_q, N_q)
    p = {n: ptr for n in "QKVOL"}
    if null:
        p[null] = None
    rc = _lib.lib().fa2_fwd_kvcache_variant(p["Q"], p["K"], p["V"], p["O"], p["L"], i64(qs), i64(ks), i64(ks), i64(qs), i64(ls),
                                            None, B, H, H_kv, N_q, S_k, d, dtype, 0, scale, window[0], window[1], num_splits, ws,
                                            ws_bytes, None, variant)
    return rc, _lib.lib().fa2_last_error().decode()


@pytest.mark.parametrize("kwargs,code,needle", [
    (dict(null="Q"), -1, "null Q"), (dict(null="K"), -1, "null K"), (dict(null="V"), -1, "null V"),
    (dict(null="O"), -1, "null O"), (dict(null="L"), -1, "null L"),
    (dict(B=0), -1, "B must"), (dict(B=65536), -1, "B must"), (dict(H=0, H_kv=1), -1, "H must"), (dict(H=65536, H_kv=1), -1, "H must"),
    (dict(H_kv=0), -1, "H_kv"), (dict(H=8, H_kv=3), -1, "H_kv"),
    (dict(N_q=0), -1, "N_q"), (dict(S_k=0), -1, "S_k"), (dict(S_k=(1 << 28) + 1), -1, "S_k"),
    (dict(B=65535, H=65535, H_kv=1, N_q=1 << 28, num_splits=128, ws=0x2000, ws_bytes=1 << 40), -1, "B * H * N_q"),
    (dict(window=(-2, 0)), -1, "window"), (dict(window=(0, -2)), -1, "window"),
    (dict(q_strides=(512, 64, -64, 1)), -1, "negative"), (dict(k_strides=(-1, 64, 64, 1)), -1, "negative"),
    (dict(l_strides=(8, -1)), -1, "negative"),
    (dict(num_splits=-1), -1, "num_splits"), (dict(num_splits=129), -1, "num_splits"),
    (dict(num_splits=4), -1, "workspace"), (dict(num_splits=4, ws=0x2000, ws_bytes=4 * 4 * 2 * 8 * 1 * 65 - 1), -1, "workspace"),
    (dict(num_splits=0, B=1, S_k=8192), -1, "workspace"),  # auto resolves to more than 1 here
    (dict(dtype=_lib.FA2_DTYPE_F8E5M2), -2, "fp8"), (dict(dtype=_lib.FA2_DTYPE_F8E4M3), -2, "fp8"), (dict(dtype=99), -2, "dtype"),
    (dict(d=0), -2, "[1, 512]"), (dict(d=513), -2, "[1, 512]"),
    (dict(variant=2, dtype=_lib.FA2_DTYPE_F32), -2, "mfma16"), (dict(variant=2, d=40), -2, "mfma16"),
    (dict(variant=2, H=40, H_kv=1, N_q=2), -2, "mfma16"), (dict(variant=2, k_strides=(2 * 512 * 128, 512 * 128, 128, 2)), -2, "mfma16"),
    (dict(variant=7), -2, "variant"),
])
def test_argument_errors_before_any_launch(kwargs, code, needle):
    rc, msg = _call(**kwargs)
    assert rc == code, (rc, msg)
    assert needle in msg, msg


def test_workspace_bytes_formula():
    for B, H, N_q, d, n in ((1, 32, 1, 128, 16), (4, 8, 5, 40, 3), (64, 32, 1, 64, 128), (3, 6, 2, 512, 2)):
        assert _lib.kvcache_workspace_bytes(B, H, N_q, d, n) == 4 * (n * B * H * N_q * d + n * B * H * N_q)
        assert _lib.kvcache_workspace_bytes(B, H, N_q, d, 1) == 0 and _lib.kvcache_workspace_bytes(B, H, N_q, d, 0) == 0


def test_split_heuristic():
    bf = _lib.FA2_DTYPE_BF16
    assert _lib.kvcache_num_splits(64, 32, 8, 1, 2048, 128, bf) == 1
    assert _lib.kvcache_num_splits(1, 32, 8, 1, 8192, 128, bf) > 1
    for H_kv in (1, 2, 8, 32):
        for S_k in (1, 63, 64, 65, 300, 4096, 8192, 131072, 1 << 28):
            prev = None
            for B in (1, 2, 3, 4, 8, 16, 31, 32, 64, 256, 65535):
                n = _lib.kvcache_num_splits(B, 32, H_kv, 1, S_k, 128, bf)
                assert 1 <= n <= 128
                assert n <= -(-S_k // KEY_TILE)
                assert prev is None or n <= prev, (H_kv, S_k, B, n, prev)
                prev = n


def test_split_heuristic_counts_the_workgroups_of_the_form_auto_takes():
    bf, f32 = _lib.FA2_DTYPE_BF16, _lib.FA2_DTYPE_F32
    # the VALU form launches one workgroup per QUERY head (and per 16 query rows): fewer splits than the matrix form at the same shape
    assert _lib.kvcache_num_splits(4, 32, 8, 1, 8192, 128, f32) < _lib.kvcache_num_splits(4, 32, 8, 1, 8192, 128, bf)
    assert _lib.kvcache_num_splits(8, 32, 8, 1, 8192, 128, f32) == 1          # 256 workgroups unsplit
    assert _lib.kvcache_num_splits(4, 32, 8, 1, 8192, 40, bf) == _lib.kvcache_num_splits(4, 32, 8, 1, 8192, 40, f32)  # d 40: VALU
    assert _lib.kvcache_num_splits(1, 32, 1, 4, 8192, 128, bf) == _lib.kvcache_num_splits(1, 32, 8, 4, 8192, 128, f32)  # g N_q = 128
    for dt in (bf, f32):
        prev = None
        for B in (1, 2, 4, 8, 64):
            n = _lib.kvcache_num_splits(B, 32, 8, 1, 8192, 128, dt)
            assert 1 <= n <= 128 and (prev is None or n <= prev)
            prev = n


def test_workspace_bytes_does_not_wrap():
    assert _lib.kvcache_workspace_bytes(65535, 65535, 1 << 28, 512, 128) in (0, 2 ** 63 - 1)  # refused or saturated, never wrapped
    assert _lib.kvcache_workspace_bytes(65535, 65535, 256, 512, 128) == 4 * 128 * 65535 * 65535 * 256 * 513


def test_python_wrapper_rejects_bad_shapes():
    Q = torch.zeros(2, 8, 1, 64, dtype=torch.bfloat16)
    K = torch.zeros(2, 2, 100, 64, dtype=torch.bfloat16)
    lens = torch.tensor([3, 5], dtype=torch.int32)
    bad = [
        dict(Q=Q[0]), dict(K=K[:1]), dict(K=K[..., :32]), dict(K=torch.zeros(2, 3, 100, 64, dtype=torch.bfloat16)),
        dict(V=K[:, :, :50]), dict(K=K.float()), dict(K=K[:, :, :0], V=K[:, :, :0]),
        dict(lens=lens.long()), dict(lens=lens[:1]), dict(lens=torch.zeros(2, 1, dtype=torch.int32)), dict(lens=[3, 5]),
        dict(window=(-2, 0)), dict(window=(1,)), dict(num_splits=-1), dict(num_splits=129), dict(num_splits=1.5),
        dict(variant="mfma16d"),
    ]
    for kw in bad:
        q, k = kw.get("Q", Q), kw.get("K", K)
        v = kw.get("V", k)
        with pytest.raises(ValueError):
            fa.flash_attention_kvcache_forward(q, k, v, kw.get("lens", lens), "cpu", window=kw.get("window"),
                                               num_splits=kw.get("num_splits", 0), variant=kw.get("variant", "auto"))
    with pytest.raises(ValueError):  # float8 caches are out of scope
        fa.flash_attention_kvcache_forward(Q.to(torch.float8_e5m2), K.to(torch.float8_e5m2), K.to(torch.float8_e5m2), lens, "cpu")


def combine(O_s, L_s):
    """The combine step as include/fa2_fwd.h and fa2_decode_combine.hip state it: O_s (S, d) normalised partials, L_s (S,) their
    log2-domain LSEs (-inf for an empty split)."""
    m = L_s.max()
    if m == -np.inf:
        return np.zeros(O_s.shape[1]), np.inf
    w = np.exp2(L_s - m)
    return (w[:, None] * O_s).sum(0) / w.sum(), m + np.log2(w.sum())


def test_combine_arithmetic_equals_unsplit_softmax():
    rng = np.random.default_rng(0)
    for trial in range(200):
        n, d = int(rng.integers(1, 300)), 16
        s = rng.normal(size=n) * 4
        v = rng.normal(size=(n, d))
        nsplit = int(rng.integers(1, 12))
        cuts = np.sort(rng.integers(0, n + 1, size=nsplit - 1))  # contiguous splits, empty ones included
        bounds = np.concatenate([[0], cuts, [n]])
        O_s, L_s = np.zeros((nsplit, d)), np.full(nsplit, -np.inf)
        for k in range(nsplit):
            lo, hi = bounds[k], bounds[k + 1]
            if hi > lo:
                mk = s[lo:hi].max()
                p = np.exp2(s[lo:hi] - mk)
                O_s[k] = p @ v[lo:hi] / p.sum()
                L_s[k] = mk + np.log2(p.sum())
        O, L = combine(O_s, L_s)
        p = np.exp2(s - s.max())
        assert np.abs(O - p @ v / p.sum()).max() <= 1e-12
        assert abs(L - (s.max() + np.log2(p.sum()))) <= 1e-12
    O, L = combine(np.zeros((3, 4)), np.full(3, -np.inf))  # every split empty
    assert (O == 0).all() and L == np.inf
