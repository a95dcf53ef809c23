"""Paged KV-cache decode (fa2_fwd_kvcache_paged), the part that needs no GPU: the exported symbol, every new argument error and
the inherited ones before any launch (fake pointers), and the Python wrapper's errors for the block table and the pools on CPU
tensors."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from conftest import ROOT

import flash_attention_dlrs_amd as fa
from flash_attention_dlrs_amd import _lib
from flash_attention_dlrs_amd.flash_attention_wrappers import check_kvcache_args


def test_symbol_exported_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "fa2_fwd.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exports = open(os.path.join(ROOT, "flash_attention_dlrs_amd", "csrc", "fa2_exports.map")).read()
    name = "fa2_fwd_kvcache_paged"
    assert name in _lib.SYMBOLS
    assert re.search(rf"\b{name}\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert re.search(rf"\bT {name}\b", out)
    assert re.search(rf"\b{name};", exports)
    assert callable(_lib.fa2_fwd_kvcache_paged)


def _call(ptr=0x1000, table=0x4000, table_stride=None, B=2, H=8, H_kv=2, N_q=1, num_blocks=32, page_size=64, max_blocks=8, d=64,
          dtype=_lib.FA2_DTYPE_BF16, kv_dtype=None, num_splits=1, ws=None, ws_bytes=0, variant=0, k_strides=None, kd=None,
          kd_strides=None):
    i64 = lambda v: None if v is None else (ctypes.c_int64 * len(v))(*v)
    qs = (H * N_q * d, N_q * d, d, 1)
    ks = k_strides or (H_kv * page_size * d, page_size * d, d, 1)
    rc = _lib.lib().fa2_fwd_kvcache_paged(ptr, ptr, ptr, ptr, ptr, i64(qs), i64(ks), i64(ks), i64(qs), i64((H * N_q, N_q)), None,
                                          table, max_blocks if table_stride is None else table_stride, kd, None, i64(kd_strides),
                                          None, B, H, H_kv, N_q, num_blocks, page_size, max_blocks, d, dtype,
                                          dtype if kv_dtype is None else kv_dtype, 0, 1.0, -1, -1, num_splits, ws, ws_bytes, variant,
                                          None)
    return rc, _lib.lib().fa2_last_error().decode()


@pytest.mark.parametrize("kwargs,code,needle", [
    # the new arguments
    (dict(table=None), -1, "null block_table"),
    (dict(page_size=0), -1, "page_size"), (dict(max_blocks=0), -1, "max_blocks"), (dict(num_blocks=0), -1, "num_blocks"),
    (dict(page_size=-64), -1, "page_size"), (dict(num_blocks=-1), -1, "num_blocks"),
    (dict(max_blocks=(1 << 22) + 1, page_size=64), -1, "2^28"),
    (dict(max_blocks=1 << 30, page_size=1 << 30), -1, "2^28"),  # the product does not fit 32 bits
    (dict(table_stride=-1), -1, "block_table_stride"),
    (dict(kd=0x3000, kd_strides=(2, 1)), -1, "descale"),  # descales with a pool in Q's dtype
    # a forced matrix form: page_size must be a multiple of 64; the message names the rule
    (dict(variant=2, page_size=48), -2, "page_size % 64"), (dict(variant=2, page_size=16), -2, "page_size % 64"),
    (dict(variant=2, page_size=48, kv_dtype=_lib.FA2_DTYPE_F8E4M3), -2, "page_size % 64"),
    # ... and the block stride is aligned like the other strides
    (dict(variant=2, k_strides=(2 * 64 * 64 + 4, 64 * 64, 64, 1)), -2, "mfma16"),
    # the workspace, counted for the capacity max_blocks * page_size
    (dict(num_splits=4), -1, "workspace"), (dict(num_splits=4, ws=0x2000, ws_bytes=4 * 4 * 2 * 8 * 1 * 65 - 1), -1, "workspace"),
    (dict(num_splits=0, B=1, max_blocks=128), -1, "workspace"),  # auto resolves to more than 1 at a capacity of 8192
    # inherited from the contiguous entry points
    (dict(ptr=None), -1, "null Q"),
    (dict(B=0), -1, "B must"), (dict(H=8, H_kv=3), -1, "H_kv"), (dict(N_q=0), -1, "N_q"),
    (dict(num_splits=129), -1, "num_splits"), (dict(k_strides=(-1, 64, 64, 1)), -1, "negative"),
    (dict(dtype=_lib.FA2_DTYPE_F8E4M3), -2, "fp8"), (dict(dtype=_lib.FA2_DTYPE_F8E5M2), -2, "fp8"),
    (dict(dtype=_lib.FA2_DTYPE_F8E4M3, kv_dtype=_lib.FA2_DTYPE_F8E5M2), -2, " dtype_enum"),
    (dict(kv_dtype=_lib.FA2_DTYPE_F32), -2, "kv_dtype_enum"), (dict(kv_dtype=99), -2, "kv_dtype_enum"),
    (dict(dtype=99), -2, "dtype"), (dict(d=513), -2, "[1, 512]"), (dict(d=0), -2, "[1, 512]"),
    (dict(variant=7), -2, "variant"), (dict(variant=2, d=40), -2, "mfma16"),
])
def test_argument_errors_before_any_launch(kwargs, code, needle):
    rc, msg = _call(**kwargs)
    assert rc == code, (rc, msg)
    assert needle in msg, msg


def test_capacity_at_the_limit_passes_the_range_check():
    """2^28 keys of capacity are accepted: the call gets as far as the workspace check of the splits the heuristic picks."""
    rc, msg = _call(max_blocks=1 << 22, page_size=64, num_splits=0)
    assert rc == -1 and "workspace" in msg, (rc, msg)


def test_python_wrapper_rejects_bad_tables_and_pools():
    Q = torch.zeros(2, 8, 1, 64, dtype=torch.bfloat16)
    pool = torch.zeros(10, 2, 16, 64, dtype=torch.bfloat16)
    table = torch.zeros(2, 4, dtype=torch.int32)
    lens = torch.tensor([3, 50], dtype=torch.int32)
    one = torch.ones(2, 2)
    bad = [
        dict(table=table.long()), dict(table=table.float()),                    # dtype
        dict(table=table[0]), dict(table=table[:, :, None]),                    # rank
        dict(table=torch.zeros(3, 4, dtype=torch.int32)),                       # the wrong B
        dict(table=torch.zeros(2, 0, dtype=torch.int32)),                       # no pages
        dict(table=torch.zeros(2, 8, dtype=torch.int32)[:, ::2]),               # non-contiguous last axis
        dict(table=torch.zeros(4, 2, dtype=torch.int32).t()),
        dict(table=[[0, 1], [2, 3]]),                                           # not a tensor
        dict(table=table.to("meta")),                                           # not Q's device
        dict(K=pool[0], V=pool[0]),                                             # pool of rank 3
        dict(V=pool[:, :, :8]), dict(V=pool[:5]),                               # K / V pools of different shape
        dict(K=pool[..., :32], V=pool[..., :32]),                               # d differs from Q's
        dict(K=pool[:, :, :0], V=pool[:, :, :0]), dict(K=pool[:0], V=pool[:0]),  # empty pools
        dict(K=torch.zeros(10, 3, 16, 64, dtype=torch.bfloat16)),               # H % H_kv != 0
        dict(K=pool.float(), V=pool.float()),                                   # dtype differs from Q's
        dict(k_descale=one), dict(v_descale=one),                               # descales with a 16-bit pool
        dict(K=pool.to(torch.float8_e4m3fn), V=pool.to(torch.float8_e5m2)),     # fp8 formats that differ
        dict(K=pool.to(torch.float8_e4m3fn), V=pool.to(torch.float8_e4m3fn), k_descale=torch.ones(3, 2)),
        dict(lens=lens.long()), dict(lens=lens[:1]),
        dict(table=torch.empty(2, (1 << 24) + 1, dtype=torch.int32, device="meta"), Q=Q.to("meta"), K=pool.to("meta"),
             V=pool.to("meta"), lens=None),                                     # capacity over 2^28
    ]
    for kw in bad:
        k = kw.get("K", pool)
        with pytest.raises(ValueError):
            fa.flash_attention_kvcache_forward(kw.get("Q", Q), k, kw.get("V", k), kw.get("lens", lens), "cpu",
                                               k_descale=kw.get("k_descale"), v_descale=kw.get("v_descale"),
                                               block_table=kw.get("table", table))
    # what is fine reaches the launch, which refuses CPU tensors: B comes from Q, not from the pool's leading axis
    wide = torch.zeros(2, 9, dtype=torch.int32)[:, 2:6]  # a column slice: row stride 9 > max_blocks
    p8 = pool.to(torch.float8_e4m3fn)
    for kw in (dict(), dict(table=wide), dict(lens=None), dict(K=p8, V=p8, k_descale=one, v_descale=torch.tensor(2.0)),
               dict(K=pool.transpose(1, 2).contiguous().transpose(1, 2), V=pool)):
        k = kw.get("K", pool)
        check_kvcache_args(Q, k, kw.get("V", k), kw.get("lens", lens), None, 1, kw.get("k_descale"), kw.get("v_descale"),
                           kw.get("table", table))
        with pytest.raises(NotImplementedError):
            fa.flash_attention_kvcache_forward(Q, k, kw.get("V", k), kw.get("lens", lens), "cpu", num_splits=1,
                                               k_descale=kw.get("k_descale"), v_descale=kw.get("v_descale"),
                                               block_table=kw.get("table", table))
    # without a table nothing changes: a pool-shaped cache is a (B, H_kv, S_k, d) cache whose B must be Q's
    with pytest.raises(ValueError):
        fa.flash_attention_kvcache_forward(Q, pool, pool, lens, "cpu")
