"""MLA decode over an fp8 latent cache (fa2_fwd_kvcache_mla_fp8), the part that needs no GPU: the exported symbol, every argument
error before any launch (fake pointers) -- what the entry point inherits from fa2_fwd_kvcache_mla and from the fp8 / paged calls, and
the fp8 rule of a forced MLA16 -- fa2_fwd_kvcache_mla's own refusal of an fp8 dtype_enum, and the Python wrapper's errors on CPU
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

NAME = "fa2_fwd_kvcache_mla_fp8"
MLA16 = 3
BF, F16, F32, F64 = _lib.FA2_DTYPE_BF16, _lib.FA2_DTYPE_F16, _lib.FA2_DTYPE_F32, _lib.FA2_DTYPE_F64
E4, E5 = _lib.FA2_DTYPE_F8E4M3, _lib.FA2_DTYPE_F8E5M2


def test_symbol_declared_bound_and_listed():
    header = open(os.path.join(ROOT, "include", "fa2_fwd.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exports = open(os.path.join(ROOT, "flash_attention_dlrs_amd", "csrc", "fa2_exports.map")).read()
    assert NAME in _lib.SYMBOLS
    assert re.search(rf"\b{NAME}\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert re.search(rf"\bT {NAME}\b", out)
    assert re.search(rf"\b{NAME};", exports)
    assert callable(_lib.fa2_fwd_kvcache_mla_fp8)
    assert _lib.KVCACHE_MLA_VARIANTS == {"auto": 0, "generic": 1, "mla16": MLA16}     # no new variant id
    assert len(_lib.lib().fa2_fwd_kvcache_mla_fp8.argtypes) == len(_lib.lib().fa2_fwd_kvcache_mla.argtypes) + 5


def _call(ptr=0x1000, v_ptr=None, null=None, table=None, table_stride=None, B=2, H=16, H_kv=1, N_q=1, num_blocks=32, page_size=512,
          max_blocks=8, d=576, d_v=512, dtype=BF, kv_dtype=E4, window=(-1, -1), num_splits=1, ws=None, ws_bytes=0, variant=0,
          k_strides=None, v_strides=None, q_strides=None, scale=1.0, kd=None, vd=None, kd_strides=(1, 1), vd_strides=(1, 1)):
    """contiguous by default (block_table null: page_size carries S_k); V aliases K unless v_ptr / v_strides say otherwise; Q, O and L
    share `ptr`, the cache has k_ptr = ptr"""
    i64 = lambda v: None if v is None else (ctypes.c_int64 * len(v))(*v)
    qs = q_strides or (H * N_q * d, N_q * d, d, 1)
    os_ = (H * N_q * d_v, N_q * d_v, d_v, 1)
    ks = k_strides or (H_kv * page_size * d, page_size * d, d, 1)
    vs = v_strides or ks
    p = {n: ptr for n in "QKVOL"}
    if v_ptr is not None:
        p["V"] = v_ptr
    if null:
        p[null] = None
    rc = _lib.lib().fa2_fwd_kvcache_mla_fp8(p["Q"], p["K"], p["V"], p["O"], p["L"], i64(qs), i64(ks), i64(vs), i64(os_),
                                            i64((H * N_q, N_q)), None, table,
                                            (max_blocks if table_stride is None else table_stride) if table else 0, kd, vd,
                                            i64(kd_strides), i64(vd_strides), B, H, H_kv, N_q, num_blocks, page_size, max_blocks, d, d_v,
                                            dtype, kv_dtype, 0, scale, window[0], window[1], num_splits, ws, ws_bytes, variant, None)
    return rc, _lib.lib().fa2_last_error().decode()


PAGED = dict(table=0x4000, page_size=64)


@pytest.mark.parametrize("kwargs,code,needle", [
    # inherited from fa2_fwd_kvcache_mla: the head sizes
    (dict(d=577), -2, "[1, 576]"), (dict(d=0), -2, "[1, 576]"), (dict(d_v=513), -2, "[1, 512]"), (dict(d_v=0), -2, "[1, 512]"),
    # ... a forced matrix form on what it cannot run
    (dict(variant=MLA16, d=128, d_v=128), -2, "d = 576"), (dict(variant=MLA16, d_v=256), -2, "d_v = 512"),
    (dict(variant=MLA16, scale=0.0), -2, "scale > 0"),
    (dict(variant=MLA16, k_strides=(512 * 1152, 512 * 1152, 1152, 2)), -2, "unit d-stride"),
    (dict(variant=2), -2, "variant"), (dict(variant=7), -2, "variant"),
    # ... the paged sizes
    (dict(PAGED, page_size=0), -1, "page_size"), (dict(PAGED, max_blocks=0), -1, "max_blocks"), (dict(PAGED, num_blocks=0), -1, "num_blocks"),
    (dict(PAGED, max_blocks=(1 << 22) + 1), -1, "2^28"), (dict(PAGED, table_stride=-1), -1, "block_table_stride"),
    (dict(page_size=0), -1, "S_k"), (dict(page_size=(1 << 28) + 1), -1, "S_k"),
    # ... the workspace on d_v, whatever the cache dtype
    (dict(num_splits=4), -1, "workspace"), (dict(num_splits=4, ws=0x2000, ws_bytes=4 * 4 * 2 * 16 * 1 * 513 - 1), -1, "workspace"),
    (dict(num_splits=0, B=1, page_size=8192), -1, "workspace"),
    (dict(PAGED, num_splits=0, B=1, max_blocks=128), -1, "workspace"),
    # ... nulls, sizes, window, strides, NaN scale
    (dict(null="Q"), -1, "null Q"), (dict(null="K"), -1, "null K"), (dict(null="V"), -1, "null V"), (dict(null="O"), -1, "null O"),
    (dict(null="L"), -1, "null L"),
    (dict(B=0), -1, "B must"), (dict(H=0), -1, "H must"), (dict(H_kv=0), -1, "H_kv"), (dict(H=16, H_kv=3), -1, "H_kv"),
    (dict(N_q=0), -1, "N_q"), (dict(window=(-2, 0)), -1, "window"), (dict(num_splits=129), -1, "num_splits"),
    (dict(k_strides=(-1, 576, 576, 1)), -1, "negative"), (dict(q_strides=(576, 576, -576, 1)), -1, "negative"),
    (dict(scale=float("nan")), -1, "NaN"),
    # the cache dtype: neither dtype_enum nor an fp8 format (fa2_fwd_kvcache_paged's code and wording)
    (dict(kv_dtype=F16), -2, "kv_dtype_enum"), (dict(kv_dtype=F32), -2, "kv_dtype_enum"), (dict(kv_dtype=99), -2, "kv_dtype_enum"),
    (dict(dtype=F16, kv_dtype=BF), -2, "FA2_DTYPE_F8E4M3 or FA2_DTYPE_F8E5M2"),
    # descales with a 16-bit cache
    (dict(kv_dtype=BF, kd=0x3000), -1, "k_descale / v_descale go with an fp8"), (dict(kv_dtype=BF, vd=0x3000), -1, "go with an fp8"),
    # negative descale strides, strides missing
    (dict(kd=0x3000, kd_strides=(-1, 1)), -1, "negative strides"), (dict(vd=0x3000, vd_strides=(1, -1)), -1, "negative strides"),
    (dict(kd=0x3000, kd_strides=None), -1, "k_descale_strides"), (dict(vd=0x3000, vd_strides=None), -1, "v_descale_strides"),
    # f32 / f64 Q under an fp8 cache; an fp8 dtype_enum
    (dict(dtype=F32), -2, "FA2_DTYPE_F16 or FA2_DTYPE_BF16"), (dict(dtype=F64, kv_dtype=E5), -2, "FA2_DTYPE_F16 or FA2_DTYPE_BF16"),
    (dict(dtype=E4, kv_dtype=E4), -2, "fp8"), (dict(dtype=E5, kv_dtype=E5), -2, "fp8"),
    # a forced MLA16 on an fp8 cache: rows 16-byte aligned in BYTES -- every stride a multiple of 16 elements, the base aligned
    (dict(variant=MLA16, k_strides=(512 * 584, 512 * 584, 584, 1)), -2, "multiple of 16 elements"),      # 8 mod 16: fine at 16 bits
    (dict(variant=MLA16, k_strides=(512 * 576 + 8, 512 * 576, 576, 1)), -2, "multiple of 16 elements"),
    (dict(variant=MLA16, kv_dtype=E5, k_strides=(512 * 576, 512 * 576 + 8, 576, 1)), -2, "multiple of 16 elements"),
    (dict(variant=MLA16, ptr=0x1008), -2, "16-byte aligned base"),
    (dict(variant=MLA16, v_ptr=0x9000), -2, "aliasing"), (dict(variant=MLA16, kv_dtype=E5, v_strides=(512 * 512, 512 * 512, 512, 1)), -2, "aliasing"),
    (dict(variant=MLA16, table=0x4000, page_size=16), -2, "page_size % 64"),
    (dict(variant=MLA16, kv_dtype=E5, table=0x4000, page_size=48), -2, "page_size % 64"),
])
def test_argument_errors_before_any_launch(kwargs, code, needle):
    rc, msg = _call(**kwargs)
    assert rc == code, (rc, msg)
    assert needle in msg, msg


def test_sixteen_bit_messages_do_not_name_the_fp8_rule():
    """the same entry point with kv_dtype_enum == dtype_enum is the 16-bit call: its forced-MLA16 message is fa2_fwd_kvcache_mla's"""
    i64 = lambda v: (ctypes.c_int64 * len(v))(*v)
    rc, msg = _call(kv_dtype=BF, variant=MLA16, k_strides=(512 * 580, 512 * 580, 580, 1))
    ks = (512 * 580, 512 * 580, 580, 1)
    rc0 = _lib.lib().fa2_fwd_kvcache_mla(0x1000, 0x1000, 0x1000, 0x1000, 0x1000, i64((16 * 576, 576, 576, 1)), i64(ks), i64(ks),
                                         i64((16 * 512, 512, 512, 1)), i64((16, 1)), None, None, 0, 2, 16, 1, 1, 32, 512, 8, 576, 512, BF,
                                         0, 1.0, -1, -1, 1, None, 0, MLA16, None)
    assert rc == rc0 == -2 and msg == _lib.lib().fa2_last_error().decode() and "fp8" not in msg and "16-byte" in msg


def test_mla_entry_point_still_refuses_an_fp8_dtype():
    i64 = lambda v: (ctypes.c_int64 * len(v))(*v)
    ks = (512 * 576, 512 * 576, 576, 1)
    for enum in (E4, E5):
        rc = _lib.lib().fa2_fwd_kvcache_mla(0x1000, 0x1000, 0x1000, 0x1000, 0x1000, i64((16 * 576, 576, 576, 1)), i64(ks), i64(ks),
                                            i64((16 * 512, 512, 512, 1)), i64((16, 1)), None, None, 0, 2, 16, 1, 1, 32, 512, 8, 576, 512,
                                            enum, 0, 1.0, -1, -1, 1, None, 0, 0, None)
        assert rc == -2 and _lib.lib().fa2_last_error().decode() == "kvcache: fp8 is not supported (e4m3fn cannot hold L = +inf)"


def test_helpers_do_not_depend_on_the_cache_dtype():
    """no new helper: the split count is asked with the I/O dtype, the workspace with d_v"""
    assert _lib.kvcache_mla_num_splits(1, 16, 1, 1, 8192, 576, 512, BF) == 32
    need = _lib.kvcache_workspace_bytes(2, 16, 1, 512, 4)
    rc, msg = _call(num_splits=4, ws=0x2000, ws_bytes=need - 1)
    assert rc == -1 and str(need) in msg


def test_python_wrapper_errors():
    Q = torch.zeros(2, 16, 1, 576, dtype=torch.bfloat16)
    KV = torch.zeros(2, 1, 128, 576, dtype=torch.bfloat16)
    lens = torch.tensor([3, 100], dtype=torch.int32)
    one = torch.ones(2, 1)
    mla = fa.flash_attention_mla_decode_forward
    for fmt in (torch.float8_e4m3fn, torch.float8_e5m2):
        KV8 = KV.to(fmt)
        # kv_descale of the wrong dtype, shape or device
        for bad in (one.double(), one.to(torch.bfloat16), torch.ones(3, 1), torch.ones(2, 2), torch.ones(2, 1, 1), 1.0,
                    torch.ones(2, 1, device="meta")):
            with pytest.raises(ValueError, match="kv_descale"):
                mla(Q, KV8, lens, "cpu", kv_descale=bad)
        # an fp8 cache under f32 / f64 Q, and under fp8 Q
        for q in (Q.float(), Q.double(), Q.to(fmt)):
            with pytest.raises(ValueError):
                mla(q, KV8, lens, "cpu")
        with pytest.raises(ValueError, match="variant"):
            mla(Q, KV8, lens, "cpu", variant="mfma16")
        # the general call keeps its refusals, and now says where an fp8 latent cache goes
        with pytest.raises(ValueError, match="fp8.*flash_attention_mla_decode_forward"):
            fa.flash_attention_kvcache_forward(Q, KV8, KV8[..., :512], lens, "cpu")
        with pytest.raises(ValueError, match="fp8"):
            fa.flash_attention_kvcache_forward(Q, KV8, KV8[..., :512], lens, "cpu", k_descale=one)
        # valid calls reach the launch, which refuses CPU tensors
        pool, table = torch.zeros(9, 1, 64, 576, dtype=torch.bfloat16).to(fmt), torch.zeros(2, 4, dtype=torch.int32)
        for kw in (dict(), dict(kv_descale=one), dict(kv_descale=torch.tensor(0.5)), dict(kv_descale=torch.ones(1, 1), variant="mla16"),
                   dict(kv_descale=torch.ones(1), variant="generic", num_splits=3, causal=True), dict(d_v=128)):
            with pytest.raises(NotImplementedError):
                mla(Q, KV8, lens, "cpu", **kw)
        with pytest.raises(NotImplementedError):
            mla(Q.to(torch.float16), pool, lens, "cpu", block_table=table, kv_descale=one, variant="mla16")
    # kv_descale with a 16-bit cache
    with pytest.raises(ValueError, match="kv_descale"):
        mla(Q, KV, lens, "cpu", kv_descale=one)
    with pytest.raises(ValueError, match="k_descale.*flash_attention_mla_decode_forward"):
        fa.flash_attention_kvcache_forward(Q, KV, KV[..., :512], lens, "cpu", k_descale=one)
    # the 16-bit call is what it was
    with pytest.raises(NotImplementedError):
        mla(Q, KV, lens, "cpu")
