"""Sparse MLA decode over the tile-scaled fp8 cache (fa2_fwd_kvcache_mla_sparse_ds, _varlen_ds) without a GPU: symbols, codes and
messages (fake pointers), the first kernel of a valid call (--forms: a child that sees no device), wrapper errors, the round trip."""
import ctypes
import json
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

NEW = ("fa2_fwd_kvcache_mla_sparse_ds", "fa2_fwd_kvcache_mla_sparse_varlen_ds")
BF16, F32 = _lib.FA2_DTYPE_BF16, _lib.FA2_DTYPE_F32


def test_symbols_declared_bound_listed_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fa2_fwd.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exports = open(os.path.join(ROOT, "flash_attention_dlrs_amd", "csrc", "fa2_exports.map")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS and re.search(rf"\b{name}\s*\(", header) and re.search(rf"\bT {name}\b", out), name
        assert re.search(rf"\b{name};", exports) and getattr(_lib.lib(), name).argtypes is not None and callable(getattr(_lib, name)), name
    for name in ("quantize_mla_cache_ds", "dequantize_mla_cache_ds"):
        assert name in fa.__all__ and callable(getattr(fa, name))


def _call(packed=False, kv=0x1000, kv_strides=(512 * 656, 512 * 656, 656), q=0x1000, dtype=BF16, variant=0, topk=200, B=3, H=16, N_q=2):
    i64 = lambda t: None if t is None else (ctypes.c_int64 * len(t))(*t)
    tail = (BF16 if dtype is None else dtype, 1.0, 1, None, 0, variant, None)
    if packed:
        rc = _lib.lib().fa2_fwd_kvcache_mla_sparse_varlen_ds(
            q, kv, 0x1000, 0x1000, i64((H * 576, 576, 1)), i64(kv_strides), i64((H * 512, 512, 1)), B * N_q, 0x6000, None, 0x3000,
            i64((topk, topk, 1)), topk, None, 0, B, H, 1, B * N_q, N_q, 0, 512, 0, *tail)
    else:
        rc = _lib.lib().fa2_fwd_kvcache_mla_sparse_ds(
            q, kv, 0x1000, 0x1000, i64((H * N_q * 576, N_q * 576, 576, 1)), i64(kv_strides), i64((H * N_q * 512, N_q * 512, 512, 1)),
            i64((H * N_q, N_q)), None, 0x3000, i64((N_q * topk, N_q * topk, topk, 1)), topk, None, 0, B, H, 1, N_q, 0, 512, 0, *tail)
    return rc, _lib.lib().fa2_last_error().decode()


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("kwargs,code,needle", [
    (dict(kv=None), -1, "fp8_ds: null KV"), (dict(kv_strides=None), -1, "fp8_ds: null kv_strides"),
    (dict(kv_strides=(512 * 656, -656, 656)), -1, "fp8_ds: negative strides are not supported (kv_strides, in bytes)"),
    (dict(dtype=F32), -2, "fp8_ds: dtype_enum"), (dict(dtype=_lib.FA2_DTYPE_F64), -2, "rotary columns of an fp8_ds row"),
    (dict(q=None), -1, "null Q"), (dict(topk=0), -1, "topk must be in [1, 2^28]"), (dict(variant=2), -2, "unknown variant 2"),
    (dict(variant=3, kv=0x1004), -2, "fp8_ds cache: needs"), (dict(variant=3, kv_strides=(512 * 660, 512 * 660, 660)), -2, "multiples of 16 bytes"),
])
def test_argument_errors_before_any_launch(kwargs, code, needle, packed):
    rc, msg = _call(packed, **kwargs)
    assert rc == code and needle in msg, (rc, msg)


def _forms():
    if torch.cuda.device_count() != 0:
        return {"skipped": "a device is visible"}
    cases = (("aligned", dict()), ("forced", dict(variant=3)), ("base4", dict(kv=0x1004)),
             ("row660", dict(kv_strides=(512 * 660, 512 * 660, 660))), ("generic", dict(variant=1)))
    return {f"{name}{int(p)}": list(_call(p, **kw)) for name, kw in cases for p in (False, True)}


def test_form_selection():
    run = subprocess.run([sys.executable, os.path.abspath(__file__), "--forms"], env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"),
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    got = json.loads(run.stdout.strip().splitlines()[-1])
    if "skipped" in got:
        pytest.skip(got["skipped"])
    for name, (rc, msg) in got.items():
        want = "kvcache mla16 kernel launch failed" if name[:-1] in ("aligned", "forced") else "kvcache mla sparse generic kernel launch failed"
        assert rc == -4 and want in msg, (name, rc, msg)


def test_python_wrapper_errors():
    bf = torch.bfloat16
    Q, KV = torch.zeros(3, 16, 2, 576, dtype=bf), torch.zeros(3, 1, 128, 656, dtype=torch.uint8)
    idx, lens = torch.zeros(3, 1, 2, 40, dtype=torch.int32), torch.tensor([3, 100, 128], dtype=torch.int32)
    cu = torch.tensor([0, 2, 3, 6], dtype=torch.int32)

    def fixed(**kw):
        return fa.flash_attention_mla_sparse_decode_forward(kw.pop("Q", Q), kw.pop("KV", KV), idx, lens, "cpu", **{"kv_format": "fp8_ds", **kw})

    def packed(**kw):
        q = kw.pop("Q", Q).transpose(1, 2).flatten(0, 1)
        return fa.flash_attention_mla_sparse_varlen_decode_forward(q, kw.pop("KV", KV), idx.transpose(1, 2).flatten(0, 1), cu, 3, lens, "cpu",
                                                                   **{"kv_format": "fp8_ds", **kw})

    for call in (fixed, packed):
        for kw, needle in ((dict(kv_format="fp8"), "kv_format must be"), (dict(KV=KV.view(torch.int8)), "torch.uint8"),
                           (dict(KV=KV[..., :576]), "656 bytes"), (dict(KV=torch.zeros(3, 1, 128, 1312, dtype=torch.uint8)[..., ::2]), "unit last"),
                           (dict(Q=Q.float()), "float16 / bfloat16"), (dict(Q=Q[..., :512]), "last axis of 576"), (dict(d_v=256), "d_v = 512"),
                           (dict(kv_descale=torch.ones(3, 1)), "no kv_descale"), (dict(KV=KV[:2]), "kvcache")):
            with pytest.raises(ValueError, match=needle):
                call(**kw)
        with pytest.raises(NotImplementedError):  # what is fine (a misaligned view too) reaches the launch, which refuses CPU tensors
            call(KV=torch.zeros(3, 1, 128, 660, dtype=torch.uint8)[..., 4:], Q=Q.half())


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=str)
def test_quantize_dequantize_round_trip(dtype):
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(2, 1, 37, 576, generator=g) * torch.exp2(torch.randint(-6, 5, (2, 1, 37, 1), generator=g).float())).to(dtype)
    x[0, 0, 1, :128] = 0  # a tile of zeros: the scale's floor
    kv8 = fa.quantize_mla_cache_ds(x)
    assert kv8.shape == (2, 1, 37, 656) and kv8.dtype == torch.uint8
    scales = kv8[..., 512:528].contiguous().view(torch.float32)
    assert (scales > 0).all() and torch.isfinite(scales).all()
    assert torch.equal(kv8[..., 528:], x[..., 512:].contiguous().view(torch.uint8))  # the rope bytes are the input's
    back = fa.dequantize_mla_cache_ds(kv8, dtype)  # within half an e4m3 step at the top binade, 2^-4 of the tile's amax
    amax = x[..., :512].float().unflatten(-1, (4, 128)).abs().amax(-1, keepdim=True)
    err = (back[..., :512].float() - x[..., :512].float()).unflatten(-1, (4, 128)).abs()
    assert (err <= amax / 16).all(), float((err - amax / 16).max())


if __name__ == "__main__":
    print(json.dumps(_forms()))
