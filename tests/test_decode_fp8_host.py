"""fp8 KV-cache decode (fa2_fwd_kvcache_fp8), the part that needs no GPU: the exported symbol, every argument error before any
launch (fake pointers), the Python wrapper's dtype and descale errors, and the quantise / dequantise helpers: the exactness of
fp8 -> f16 / bf16 that the kernels' descale fold rests on, the round trip's error and the all-zero head."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from conftest import ROOT

import flash_attention_dlrs_amd as fa
from flash_attention_dlrs_amd import _lib

FP8 = (torch.float8_e4m3fn, torch.float8_e5m2)


def test_symbol_exported_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "fa2_fwd.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    name = "fa2_fwd_kvcache_fp8"
    assert name in _lib.SYMBOLS
    assert re.search(rf"\b{name}\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert re.search(rf"\bT {name}\b", out)
    assert fa.quantize_kv_cache is not None and fa.dequantize_kv_cache is not None
    assert "quantize_kv_cache" in fa.__all__ and "dequantize_kv_cache" in fa.__all__


def _call(ptr=0x1000, null=None, B=2, H=8, H_kv=2, N_q=1, S_k=512, d=64, dtype=_lib.FA2_DTYPE_BF16, kv_dtype=_lib.FA2_DTYPE_F8E4M3,
          window=(-1, -1), num_splits=1, ws=None, ws_bytes=0, variant=0, q_strides=None, k_strides=None, l_strides=None, scale=1.0,
          kd=None, vd=None, kd_strides=None, vd_strides=None):
    i64 = lambda v: None if v is None else (ctypes.c_int64 * len(v))(*v)
    qs = q_strides or (H * N_q * d, N_q * d, d, 1)
    ks = k_strides or (H_kv * S_k * d, S_k * d, d, 1)
    ls = l_strides or (H * N_q, N_q)
    p = {n: ptr for n in "QKVOL"}
    if null in p:
        p[null] = None
    st = {"q_strides": i64(qs), "k_strides": i64(ks), "v_strides": i64(ks), "o_strides": i64(qs), "l_strides": i64(ls)}
    if null in st:
        st[null] = None
    rc = _lib.lib().fa2_fwd_kvcache_fp8(p["Q"], p["K"], p["V"], p["O"], p["L"], st["q_strides"], st["k_strides"], st["v_strides"],
                                        st["o_strides"], st["l_strides"], None, kd, vd, i64(kd_strides), i64(vd_strides), B, H,
                                        H_kv, N_q, S_k, d, dtype, kv_dtype, 0, scale, window[0], window[1], num_splits, ws,
                                        ws_bytes, variant, None)
    return rc, _lib.lib().fa2_last_error().decode()


@pytest.mark.parametrize("kwargs,code,needle", [
    # every FA2_ERR_BAD_ARG of fa2_fwd_kvcache, the same argument names (tests/test_decode_host.py)
    (dict(null="Q"), -1, "null Q"), (dict(null="K"), -1, "null K"), (dict(null="V"), -1, "null V"),
    (dict(null="O"), -1, "null O"), (dict(null="L"), -1, "null L"),
    (dict(null="q_strides"), -1, "null q_strides"), (dict(null="k_strides"), -1, "null k_strides"),
    (dict(null="v_strides"), -1, "null v_strides"), (dict(null="o_strides"), -1, "null o_strides"),
    (dict(null="l_strides"), -1, "null l_strides"),
    (dict(B=0), -1, "B must"), (dict(B=65536), -1, "B must"), (dict(H=0, H_kv=1), -1, "H must"), (dict(H=65536, H_kv=1), -1, "H must"),
    (dict(H_kv=0), -1, "H_kv"), (dict(H=8, H_kv=3), -1, "H_kv"),
    (dict(N_q=0), -1, "N_q"), (dict(S_k=0), -1, "S_k"), (dict(S_k=(1 << 28) + 1), -1, "S_k"),
    (dict(B=65535, H=65535, H_kv=1, N_q=1 << 28, num_splits=128, ws=0x2000, ws_bytes=1 << 40), -1, "B * H * N_q"),
    (dict(window=(-2, 0)), -1, "window"), (dict(window=(0, -2)), -1, "window"),
    (dict(q_strides=(512, 64, -64, 1)), -1, "negative"), (dict(k_strides=(-1, 64, 64, 1)), -1, "negative"),
    (dict(l_strides=(8, -1)), -1, "negative"), (dict(scale=float("nan")), -1, "NaN"),
    (dict(num_splits=-1), -1, "num_splits"), (dict(num_splits=129), -1, "num_splits"),
    (dict(num_splits=4), -1, "workspace"), (dict(num_splits=4, ws=0x2000, ws_bytes=4 * 4 * 2 * 8 * 1 * 65 - 1), -1, "workspace"),
    (dict(num_splits=0, B=1, S_k=8192), -1, "workspace"),  # auto resolves to more than 1 here, as for a bf16 cache
    # the descales
    (dict(kd=0x3000), -1, "k_descale_strides"), (dict(vd=0x3000), -1, "v_descale_strides"),
    (dict(kd=0x3000, kd_strides=(2, 1), vd=0x3000), -1, "v_descale_strides"),
    (dict(kd=0x3000, kd_strides=(-2, 1)), -1, "negative"), (dict(kd=0x3000, kd_strides=(2, -1)), -1, "negative"),
    (dict(vd=0x3000, vd_strides=(0, -1)), -1, "negative"), (dict(vd=0x3000, vd_strides=(-1, 0)), -1, "negative"),
    # unsupported, the argument named
    (dict(kv_dtype=_lib.FA2_DTYPE_BF16), -2, "kv_dtype_enum"), (dict(kv_dtype=_lib.FA2_DTYPE_F16), -2, "kv_dtype_enum"),
    (dict(kv_dtype=_lib.FA2_DTYPE_F32), -2, "kv_dtype_enum"), (dict(kv_dtype=99), -2, "kv_dtype_enum"),
    (dict(dtype=_lib.FA2_DTYPE_F32), -2, " dtype_enum"), (dict(dtype=_lib.FA2_DTYPE_F64), -2, " dtype_enum"),
    (dict(dtype=_lib.FA2_DTYPE_F8E4M3), -2, " dtype_enum"), (dict(dtype=_lib.FA2_DTYPE_F8E5M2), -2, " dtype_enum"),
    (dict(dtype=99), -2, " dtype_enum"),
    (dict(d=0), -2, "[1, 512]"), (dict(d=513), -2, "[1, 512]"),
    (dict(variant=7), -2, "variant"),
    # a forced matrix form on what it cannot take: d, g * N_q, a non-unit d-stride, rows that are not 16 fp8 elements apart
    (dict(variant=2, d=40), -2, "mfma16"), (dict(variant=2, H=40, H_kv=1, N_q=2), -2, "mfma16"),
    (dict(variant=2, k_strides=(2 * 512 * 128, 512 * 128, 128, 2)), -2, "mfma16"),
    (dict(variant=2, k_strides=(2 * 512 * 72, 512 * 72, 72, 1)), -2, "mfma16"),
])
def test_argument_errors_before_any_launch(kwargs, code, needle):
    rc, msg = _call(**kwargs)
    assert rc == code, (rc, msg)
    assert needle in msg, msg


def test_sixteen_bit_entry_points_still_refuse_fp8():
    i64 = lambda v: (ctypes.c_int64 * len(v))(*v)
    for dt in (_lib.FA2_DTYPE_F8E4M3, _lib.FA2_DTYPE_F8E5M2):
        rc = _lib.lib().fa2_fwd_kvcache(0x1000, 0x1000, 0x1000, 0x1000, 0x1000, i64((512, 64, 64, 1)), i64((65536, 32768, 64, 1)),
                                        i64((65536, 32768, 64, 1)), i64((512, 64, 64, 1)), i64((8, 1)), None, 2, 8, 2, 1, 512, 64, dt,
                                        0, 1.0, -1, -1, 1, None, 0, None)
        assert rc == -2 and "fp8" in _lib.lib().fa2_last_error().decode()


def test_python_wrapper_rejects_bad_dtypes_and_descales():
    Q = torch.zeros(2, 8, 1, 64, dtype=torch.bfloat16)
    K = torch.zeros(2, 2, 100, 64, dtype=torch.bfloat16)
    K8, K5 = K.to(torch.float8_e4m3fn), K.to(torch.float8_e5m2)
    lens = torch.tensor([3, 5], dtype=torch.int32)
    one = torch.ones(2, 2)
    bad = [
        dict(K=K, V=K, k_descale=one), dict(K=K, V=K, v_descale=one),           # descales with a 16-bit cache
        dict(K=K8, V=K5), dict(K=K5, V=K8), dict(K=K8, V=K), dict(K=K, V=K8),   # K / V formats that differ
        dict(Q=Q.to(torch.float8_e4m3fn), K=K8, V=K8), dict(Q=Q.to(torch.float8_e5m2), K=K5, V=K5),  # fp8 Q
        dict(Q=Q.float(), K=K8, V=K8), dict(Q=Q.double(), K=K5, V=K5),          # Q must be 16-bit over an fp8 cache
        dict(K=K.float(), V=K.float()),                                         # f32 cache under bf16 Q, as before
        dict(K=K8, V=K8, k_descale=one.double()), dict(K=K8, V=K8, v_descale=one.to(torch.bfloat16)),
        dict(K=K8, V=K8, k_descale=[1.0]), dict(K=K8, V=K8, v_descale=1.0),
        dict(K=K8, V=K8, k_descale=torch.ones(3, 2)), dict(K=K8, V=K8, v_descale=torch.ones(2, 3)),
        dict(K=K8, V=K8, k_descale=torch.ones(2, 2, 1)), dict(K=K5, V=K5, v_descale=torch.ones(4)),
        dict(K=K8, V=K8, k_descale=one.to("meta")),                             # not Q's device
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            fa.flash_attention_kvcache_forward(kw.get("Q", Q), kw["K"], kw["V"], lens, "cpu", k_descale=kw.get("k_descale"),
                                               v_descale=kw.get("v_descale"))
    # what is fine reaches the launch, which refuses CPU tensors
    for kw in (dict(), dict(k_descale=one), dict(v_descale=torch.tensor(2.0)), dict(k_descale=torch.ones(1, 1), v_descale=torch.ones(2, 1)),
               dict(k_descale=torch.ones(2))):
        with pytest.raises(NotImplementedError):
            fa.flash_attention_kvcache_forward(Q, K8, K8, lens, "cpu", num_splits=1, **kw)


@pytest.mark.parametrize("fmt", FP8)
@pytest.mark.parametrize("wide", [torch.float16, torch.bfloat16])
def test_every_finite_byte_converts_exactly(fmt, wide):
    """fp8 -> f16 / bf16 is exact: each of the 256 byte patterns that is finite converts and comes back as the same byte, and its
    16-bit value equals its fp32 value."""
    b = torch.arange(256, dtype=torch.int16).to(torch.uint8)
    x = b.view(fmt)
    finite = torch.isfinite(x.float())
    assert int(finite.sum()) == {torch.float8_e4m3fn: 254, torch.float8_e5m2: 248}[fmt]
    w = x.to(wide)
    assert torch.equal(w.float()[finite], x.float()[finite])
    assert torch.equal(w.to(fmt).view(torch.uint8)[finite], b[finite])


@pytest.mark.parametrize("fmt,half_ulp,min_normal", [(torch.float8_e4m3fn, 2.0 ** -4, 2.0 ** -6), (torch.float8_e5m2, 2.0 ** -3, 2.0 ** -14)])
def test_quantize_round_trip(fmt, half_ulp, min_normal):
    g = torch.Generator().manual_seed(0)
    K = torch.randn(3, 4, 200, 64, generator=g) * torch.tensor([0.01, 0.5, 3.0, 100.0]).view(1, 4, 1, 1)
    K[1, 2] = 0
    K8, ds = fa.quantize_kv_cache(K, fmt)
    assert K8.dtype == fmt and K8.shape == K.shape and ds.dtype == torch.float32 and ds.shape == (3, 4)
    assert ds[1, 2] == 1 and (K8[1, 2].float() == 0).all()                       # an all-zero head: descale 1
    amax = K.abs().amax(dim=(2, 3))
    keep = amax > 0
    assert torch.equal(ds[keep], (amax / torch.finfo(fmt).max)[keep]) and (ds > 0).all()
    assert torch.isfinite(K8.float()).all() and K8.float().abs().max() == torch.finfo(fmt).max
    back = fa.dequantize_kv_cache(K8, ds, torch.float32)
    assert back.dtype == torch.float32
    assert torch.equal(back, K8.float() * ds[:, :, None, None])
    normal = (K.abs() / ds[:, :, None, None]) >= min_normal                       # values the format holds as normal numbers
    err = (back.double() - K.double()).abs()
    assert normal.float().mean() > 0.9
    assert (err[normal] <= half_ulp * K.double().abs()[normal]).all()
    # 16-bit caches, a broadcast descale, and bad arguments
    Kb = K.to(torch.bfloat16)
    K8b, dsb = fa.quantize_kv_cache(Kb, fmt)
    assert fa.dequantize_kv_cache(K8b, dsb, torch.bfloat16).dtype == torch.bfloat16
    assert torch.equal(fa.dequantize_kv_cache(K8, torch.tensor(2.0), torch.float32), K8.float() * 2)
    with pytest.raises(ValueError):
        fa.quantize_kv_cache(K, torch.float16)
    with pytest.raises(ValueError):
        fa.quantize_kv_cache(K[0], fmt)
