"""Packed MLA decode with fp8 queries (fa2_fwd_kvcache_mla_varlen_q8) without a GPU: symbols, argument errors, split rule, wrapper errors."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from conftest import ROOT

import flash_attention_dlrs_amd as fa
from flash_attention_dlrs_amd import _lib

MLA8 = 4
BF, F32, E4, E5 = _lib.FA2_DTYPE_BF16, _lib.FA2_DTYPE_F32, _lib.FA2_DTYPE_F8E4M3, _lib.FA2_DTYPE_F8E5M2


@pytest.mark.parametrize("name", ["fa2_fwd_kvcache_mla_varlen_q8", "fa2_kvcache_mla_varlen_q8_num_splits"])
def test_symbols_declared_bound_and_listed(name):
    header = open(os.path.join(ROOT, "include", "fa2_fwd.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exports = open(os.path.join(ROOT, "flash_attention_dlrs_amd", "csrc", "fa2_exports.map")).read()
    assert name in _lib.SYMBOLS and re.search(rf"\b{name}\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert re.search(rf"\bT {name}\b", out) and re.search(rf"\b{name};", exports)
    assert _lib.KVCACHE_MLA_Q8_VARIANTS == {"auto": 0, "generic": 1, "mla8": MLA8}
    for py in ("flash_attention_mla_varlen_decode_q8_forward", "check_mla_varlen_q8_args"):
        assert py in fa.__all__ and callable(getattr(fa, py))


def _call(ptr=0x1000, table=None, B=2, H=16, total_q=5, max_q=4, S_k=512, page_size=64, d=576, d_v=512, dtype=BF, kv_dtype=E4, q_dtype=E4,
          num_splits=1, ws=None, ws_bytes=0, variant=0, q_strides=None, cu=0x5000, l_stride=None, qd=None, qd_strides=(1, 1)):
    i64 = lambda v: None if v is None else (ctypes.c_int64 * len(v))(*v)
    rows = page_size if table else S_k
    rc = _lib.lib().fa2_fwd_kvcache_mla_varlen_q8(ptr, ptr, ptr, ptr, i64(q_strides or (H * d, d, 1)), i64((rows * d, rows * d, d, 1)),
                                                  i64((H * d_v, d_v, 1)), total_q if l_stride is None else l_stride, cu, None, table,
                                                  8 if table else 0, None, None, qd, i64(qd_strides), B, H, 1, total_q, max_q, S_k, 32,
                                                  page_size, 8, d, d_v, dtype, kv_dtype, q_dtype, 0, 1.0, -1, -1, num_splits, ws, ws_bytes,
                                                  variant, None)
    return rc, _lib.lib().fa2_last_error().decode()


@pytest.mark.parametrize("kwargs,code,needle", [
    # the dtypes and the query's descale; the packed queries; the variants of this call and the rule a forced MLA8 names; the workspace
    (dict(q_dtype=BF), -2, "q_dtype_enum"), (dict(kv_dtype=BF), -2, "kv_dtype_enum"),
    (dict(dtype=F32), -2, "(O) must be FA2_DTYPE_F16 or FA2_DTYPE_BF16"), (dict(dtype=E4), -2, "(O) must be"),
    (dict(qd=0x3000, qd_strides=None), -1, "q_descale_strides"), (dict(qd=0x3000, qd_strides=(1, -1)), -1, "q_descale_strides"),
    (dict(cu=None), -1, "null cu_seqlens_q"), (dict(total_q=0), -1, "total_q must be >= 1"), (dict(max_q=0), -1, "max_seqlen_q must be in"),
    (dict(l_stride=-1), -1, "l_head_stride"),
    (dict(variant=3), -2, "mla8 4"), (dict(variant=2), -2, "mla8 4"),
    (dict(variant=MLA8, table=0x4000, page_size=16), -2, "page_size % 64"),
    (dict(variant=MLA8, q_dtype=E5), -2, "e4m3fn Q over an e4m3fn cache"), (dict(variant=MLA8, kv_dtype=E5), -2, "e4m3fn Q over an e4m3fn cache"),
    (dict(variant=MLA8, d=192, d_v=128), -2, "d = 576 and d_v = 512"),
    (dict(variant=MLA8, q_strides=(16 * 584, 584, 1)), -2, "multiples of 16 bytes"), (dict(variant=MLA8, ptr=0x1008), -2, "16-byte aligned"),
    (dict(num_splits=4), -1, "workspace"), (dict(num_splits=0, B=1, total_q=1, max_q=1, S_k=8192), -1, "workspace"),
    (dict(num_splits=4, ws=0x2000, ws_bytes=4 * 4 * 5 * 16 * 513 - 1), -1, str(4 * 4 * 5 * 16 * 513)),
])
def test_argument_errors_before_any_launch(kwargs, code, needle):
    rc, msg = _call(**kwargs)
    assert rc == code and needle in msg, (rc, msg)


@pytest.mark.parametrize("shape", [(1, 16, 1, 1, 1, 8192), (4, 128, 1, 9, 4, 8192), (64, 16, 1, 319, 256, 4096), (3, 72, 2, 11, 5, 256)])
def test_split_rule(shape):
    q8, v16 = _lib.kvcache_mla_varlen_q8_num_splits, _lib.kvcache_mla_varlen_num_splits  # (F32, d 192: counted as the VALU form's)
    assert q8(*shape, 576, 512, E4, E4) == v16(*shape, 576, 512, BF)
    assert q8(*shape, 576, 512, E5, E4) == q8(*shape, 576, 512, E4, E5) == v16(*shape, 576, 512, F32)
    assert q8(*shape, 192, 128, E4, E4) == v16(*shape, 192, 128, BF) and q8(0, *shape[1:], 576, 512, E4, E4) == 1


def test_python_wrapper_errors():
    e4, e5 = torch.float8_e4m3fn, torch.float8_e5m2
    Q, KV = torch.zeros(5, 16, 576).to(e4), torch.zeros(2, 1, 128, 576).to(e4)
    cu, lens, one = torch.tensor([0, 2, 5], dtype=torch.int32), torch.tensor([3, 100], dtype=torch.int32), torch.ones(2, 1)
    q8 = fa.flash_attention_mla_varlen_decode_q8_forward
    for bad in (dict(Q8=Q.to(torch.bfloat16)), dict(Q8=Q[None]), dict(KV_cache=KV.to(torch.bfloat16)), dict(KV_cache=KV[..., :512]),
                dict(d_v=576), dict(out_dtype=torch.float32), dict(variant="mla16"), dict(num_splits=129), dict(window=(-2, 0)),
                dict(q_descale=one.double()), dict(q_descale=torch.ones(3, 1)), dict(kv_descale=1.0), dict(kv_descale=torch.ones(2, 2)),
                dict(cu_seqlens_q=cu.long()), dict(cu_seqlens_q=cu[:1]), dict(max_seqlen_q=0), dict(cache_seqlens=lens.long()),
                dict(block_table=torch.zeros(2, 4))):
        with pytest.raises(ValueError):
            q8(**dict(dict(Q8=Q, KV_cache=KV, cu_seqlens_q=cu, max_seqlen_q=3, cache_seqlens=lens, dev="cpu"), **bad))
    # valid calls reach the launch, which refuses CPU tensors; the 16-bit packed call keeps refusing fp8 Q
    for kw in (dict(), dict(q_descale=one, kv_descale=torch.tensor(0.5), variant="mla8"), dict(out_dtype=torch.float16, causal=True, num_splits=3),
               dict(d_v=128, variant="generic")):
        with pytest.raises(NotImplementedError):
            q8(Q, KV.to(e5) if "d_v" in kw else KV, cu, 3, lens, "cpu", **kw)
    with pytest.raises(ValueError):
        fa.flash_attention_mla_varlen_decode_forward(Q, KV, cu, 3, lens, "cpu")
