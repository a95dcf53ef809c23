"""The quantising appends (fa2_kvcache_mla_append_ds, fa2_mla_indexer_append and their _varlen forms) without a GPU: symbols, the C
entry points' codes and messages (fake pointers, nothing is launched), the wrappers' errors and which launcher a call reaches."""
import ctypes
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import pytest
import torch

import flash_attention_dlrs_amd as fa
from flash_attention_dlrs_amd import _lib

NEW = ("fa2_kvcache_mla_append_ds", "fa2_kvcache_mla_append_varlen_ds", "fa2_mla_indexer_append", "fa2_mla_indexer_append_varlen")
BF16, F32, E4 = _lib.FA2_DTYPE_BF16, _lib.FA2_DTYPE_F32, _lib.FA2_DTYPE_F8E4M3
i64 = lambda t: None if t is None else (ctypes.c_int64 * len(t))(*t)


def test_symbols_declared_bound_listed_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fa2_fwd.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exports = open(os.path.join(ROOT, "flash_attention_dlrs_amd", "csrc", "fa2_exports.map")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS and re.search(rf"\b{name}\s*\(", header) and re.search(rf"\bT {name}\b", out), name
        assert re.search(rf"\b{name};", exports) and getattr(_lib.lib(), name).argtypes is not None, name


def _ds(packed, kv=0x1000, kv_strides=(192 * 656, 192 * 656, 656), c_new=0x2000, out=0x5000, dtype=BF16, rd=64, B=3):
    rot = (0x6000, 0x7000, 32, 32, 100, rd, 0)
    if packed:
        rc = _lib.lib().fa2_kvcache_mla_append_varlen_ds(kv, i64(kv_strides), None, 0, c_new, 0x3000, i64((512, 512, 1)), i64((64, 64, 1)),
                                                         0x8000, 0x4000, out, *rot, B, 1, 9, 4, 192, 0, 0, 0, dtype, None)
    else:
        rc = _lib.lib().fa2_kvcache_mla_append_ds(kv, i64(kv_strides), None, 0, c_new, 0x3000, i64((512, 512, 512, 1)), i64((64, 64, 64, 1)),
                                                  0x4000, out, *rot, B, 1, 1, 192, 0, 0, 0, dtype, None)
    return rc, _lib.lib().fa2_last_error().decode()


def _idx(packed, k_idx=0x1000, k_scale=0x2000, k_new=0x3000, out=0x5000, dtype=BF16, k_dtype=E4, d_I=128, k_strides=(192 * 128, 128, 1)):
    head = (k_idx, i64(k_strides), k_scale, i64((192, 1)), None, 0, k_new)
    if packed:
        rc = _lib.lib().fa2_mla_indexer_append_varlen(*head, i64((d_I, 1)), 0x8000, 0x4000, out, 3, 9, 4, 192, 0, 0, 0, d_I, dtype, k_dtype, None)
    else:
        rc = _lib.lib().fa2_mla_indexer_append(*head, i64((d_I, d_I, 1)), 0x4000, out, 3, 1, 192, 0, 0, 0, d_I, dtype, k_dtype, None)
    return rc, _lib.lib().fa2_last_error().decode()


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("call,kwargs,code,needle", [
    (_ds, dict(kv=None), -1, "null KV"), (_ds, dict(kv_strides=None), -1, "null kv_strides"), (_ds, dict(c_new=None), -1, "null c_new"),
    (_ds, dict(kv_strides=(656, -656, 656)), -1, "negative strides"), (_ds, dict(out=0x4000), -1, "seqlens_out must not be cache_seqlens"),
    (_ds, dict(dtype=F32), -2, "must be FA2_DTYPE_F16 or FA2_DTYPE_BF16"), (_ds, dict(rd=66), -1, "rotary_dim must be even and in [2, d - d_v = 64]"),
    (_ds, dict(B=0), -1, "B must be in [1, 65535]"),
    (_idx, dict(k_idx=None), -1, "null k_idx"), (_idx, dict(k_new=None), -1, "null k_new"), (_idx, dict(k_scale=None), -1, "null k_scale with an fp8 cache"),
    (_idx, dict(k_dtype=BF16), -1, "k_scale goes with an fp8 cache"), (_idx, dict(dtype=F32), -2, "goes with f16 / bf16 k_new, not f32"),
    (_idx, dict(d_I=577), -2, "d_I=577 must be in [1, 576]"), (_idx, dict(k_strides=(128, -1, 1)), -1, "negative strides"),
    (_idx, dict(out=0x4000), -1, "must not be cache_seqlens"),
])
def test_argument_errors_before_any_launch(call, kwargs, code, needle, packed):
    rc, msg = call(packed, **kwargs)
    assert rc == code and needle in msg, (rc, msg)


def test_kv_format_wrapper_errors_name_their_argument():
    KV, lens = torch.zeros(3, 1, 192, 656, dtype=torch.uint8), torch.zeros(3, dtype=torch.int32)
    new, cu = torch.zeros(3, 1, 1, 576, dtype=torch.bfloat16), torch.tensor([0, 1, 2, 3], dtype=torch.int32)

    def fixed(KV=KV, new=new, **kw):
        return fa.mla_kvcache_append(KV, new, lens, **{"kv_format": "fp8_ds", **kw})

    def packed(KV=KV, new=new, **kw):
        new = tuple(t[:, :, 0] for t in new) if isinstance(new, tuple) else new[:, :, 0]
        return fa.mla_kvcache_append_varlen(KV, new, cu, 1, lens, **{"kv_format": "fp8_ds", **kw})

    for call in (fixed, packed):
        for kw, needle in ((dict(kv_format="fp8"), "kv_format must be"), (dict(KV=KV.view(torch.int8)), "KV_cache in torch.uint8"),
                           (dict(KV=KV[..., :576]), "656 bytes"), (dict(d_v=256), "d_v = 512"),
                           (dict(kv_descale=torch.ones(3, 1)), "no kv_descale"), (dict(new=new.float()), "needs kv_new in float16 / bfloat16"),
                           (dict(new=(new[..., :512], new[..., :32])), "kv_new"), (dict(KV=KV[:2]), "kv_new must be|cu_seqlens_new's B = 3")):
            with pytest.raises(ValueError, match=needle):
                call(**kw)
        with pytest.raises(NotImplementedError):  # what is fine (the pair, a misaligned cache view) reaches the launch, which refuses CPU tensors
            call(KV=torch.zeros(3, 1, 192, 660, dtype=torch.uint8)[..., 4:], new=(new[..., :512].half(), new[..., 512:].half()))


def test_indexer_append_wrapper_errors_name_their_argument():
    k8, ks, lens = torch.zeros(3, 192, 128, dtype=torch.float8_e4m3fn), torch.zeros(3, 192), torch.zeros(3, dtype=torch.int32)
    new, cu = torch.zeros(3, 1, 128, dtype=torch.bfloat16), torch.tensor([0, 1, 2, 3], dtype=torch.int32)

    def fixed(k=k8, new=new, **kw):
        return fa.mla_indexer_append(k, new, lens, **{"k_scale": ks, **kw})

    def packed(k=k8, new=new, **kw):
        return fa.mla_indexer_append_varlen(k, new[:, 0], cu, 1, lens, **{"k_scale": ks, **kw})

    for call in (fixed, packed):
        for kw, needle in ((dict(k_scale=None), "needs its k_scale"), (dict(k=k8.to(torch.bfloat16)), "k_scale goes with an fp8 k_idx"),
                           (dict(new=new.float()), "float16 / bfloat16 k_new, not float32"), (dict(new=new[..., :96]), "k_idx's d_I = 128"),
                           (dict(k=k8.to(torch.float16), k_scale=None), "k_idx must have k_new's dtype"),
                           (dict(k_scale=ks[:, :100]), "k_scale must be a float32 tensor shaped like"), (dict(k=k8[:2], k_scale=ks[:2]), "B = 3")):
            with pytest.raises(ValueError, match=needle):
                call(**kw)
        for kw in (dict(), dict(k=k8.to(torch.bfloat16), k_scale=None)):
            with pytest.raises(NotImplementedError):
                call(**kw)


def test_kv_format_none_reaches_the_old_symbols(monkeypatch):
    seen = []
    for name in ("fa2_kvcache_mla_append", "fa2_kvcache_mla_append_varlen", "fa2_kvcache_mla_append_ds"):
        monkeypatch.setattr(_lib, name, lambda *a, _n=name, **k: seen.append((_n, k.get("cu_new") is not None)))
    lens, cu = torch.zeros(3, dtype=torch.int32), torch.tensor([0, 1, 2, 3], dtype=torch.int32)
    new = torch.zeros(3, 1, 1, 576, dtype=torch.bfloat16)
    for kv, kw in ((torch.zeros(3, 1, 192, 576, dtype=torch.bfloat16), dict()), (torch.zeros(3, 1, 192, 656, dtype=torch.uint8), dict(kv_format="fp8_ds"))):
        fa.mla_kvcache_append(kv, new, lens, **kw)
        fa.mla_kvcache_append_varlen(kv, new[:, :, 0], cu, 1, lens, **kw)
    assert seen == [("fa2_kvcache_mla_append", False), ("fa2_kvcache_mla_append_varlen", False), ("fa2_kvcache_mla_append_ds", False),
                    ("fa2_kvcache_mla_append_ds", True)]
