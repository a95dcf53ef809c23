"""The packed (ragged) KV-cache append (fa2_kvcache_append_varlen, fa2_fwd_kvcache_varlen_append), the part that needs no GPU: the
exported symbols, every argument error of both entry points before any launch (fake pointers), and the Python wrappers' errors on
CPU tensors."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from conftest import ROOT

import flash_attention_dlrs_amd as fa
from flash_attention_dlrs_amd import _lib
from flash_attention_dlrs_amd.flash_attention_wrappers import (check_kvcache_append_varlen_args, check_varlen_kvcache_args)

F8E4, F8E5, F32, BF16 = _lib.FA2_DTYPE_F8E4M3, _lib.FA2_DTYPE_F8E5M2, _lib.FA2_DTYPE_F32, _lib.FA2_DTYPE_BF16


def test_symbols_exported_declared_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fa2_fwd.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exports = open(os.path.join(ROOT, "flash_attention_dlrs_amd", "csrc", "fa2_exports.map")).read()
    for name in ("fa2_kvcache_append_varlen", "fa2_fwd_kvcache_varlen_append"):
        assert name in _lib.SYMBOLS
        assert re.search(rf"\b{name}\s*\(", header)
        assert re.search(rf"\bT {name}\b", out)
        assert re.search(rf"\b{name};", exports)
        assert callable(getattr(_lib, name)) and getattr(_lib.lib(), name) is not None
    assert "kvcache_append_varlen" in fa.__all__ and callable(fa.kvcache_append_varlen)


def _i64(v):
    return None if v is None else (ctypes.c_int64 * len(v))(*v)


def _args(ptr=0x1000, K=0x1000, k_new=0x2000, v_new=0x2000, cu=0x2800, lens=0x3000, out=0x3100, table=None, table_stride=8, B=2, H=8,
          H_kv=2, total=5, max_new=3, S_k=256, num_blocks=32, page_size=64, max_blocks=8, d=64, dtype=BF16, kv_dtype=None, kd=None,
          kd_strides=None, cos=None, sin=None, cos_stride=32, S_rot=512, rotary_dim=64, Q=0x5000, q_rot=0x6000, k_strides=None,
          kn_strides=None, q_strides=None, o_strides=(512, 64, 1), l_stride=5, num_splits=1, variant=0, wl=-1):
    a = dict(locals())
    a["k_strides"] = _i64(k_strides or (H_kv * 256 * d, 256 * d, d, 1))
    a["kn_strides"] = _i64(kn_strides or (H_kv * d, d, 1))
    a["q_strides"] = _i64(q_strides or (H * d, d, 1))
    a["kv_dtype"] = dtype if kv_dtype is None else kv_dtype
    return a


def _append(**kw):
    no_q_strides = kw.pop("null_q_strides", False)
    a = _args(**kw)
    rc = _lib.lib().fa2_kvcache_append_varlen(a["K"], a["ptr"], a["k_strides"], a["k_strides"], a["table"], a["table_stride"], a["k_new"],
                                              a["v_new"], a["kn_strides"], a["kn_strides"], a["cu"], a["lens"], a["out"], a["kd"], None,
                                              _i64(a["kd_strides"]), None, a["cos"], a["sin"], a["cos_stride"], a["cos_stride"],
                                              a["S_rot"], a["rotary_dim"], 0, a["Q"], a["q_rot"], None if no_q_strides else a["q_strides"],
                                              a["H"], 0, a["B"], a["H_kv"], a["total"], a["max_new"], a["S_k"], a["num_blocks"],
                                              a["page_size"], a["max_blocks"], a["d"], a["dtype"], a["kv_dtype"], None)
    return rc, _lib.lib().fa2_last_error().decode()


def _fused(**kw):
    no_q_strides = kw.pop("null_q_strides", False)
    a = _args(**kw)
    rc = _lib.lib().fa2_fwd_kvcache_varlen_append(a["Q"], a["K"], a["ptr"], a["ptr"], a["ptr"], None if no_q_strides else a["q_strides"],
                                                  a["k_strides"], a["k_strides"], _i64(a["o_strides"]), a["l_stride"], a["cu"], a["lens"],
                                                  a["out"], a["table"], a["table_stride"], a["kd"], None, _i64(a["kd_strides"]), None,
                                                  a["k_new"], a["v_new"], a["kn_strides"], a["kn_strides"], a["cos"], a["sin"],
                                                  a["cos_stride"], a["cos_stride"], a["S_rot"], a["rotary_dim"], 0, a["q_rot"], a["B"],
                                                  a["H"], a["H_kv"], a["total"], a["max_new"], a["S_k"], a["num_blocks"], a["page_size"],
                                                  a["max_blocks"], a["d"], a["dtype"], a["kv_dtype"], 0, 1.0, a["wl"], -1,
                                                  a["num_splits"], None, 0, a["variant"], None)
    return rc, _lib.lib().fa2_last_error().decode()


ROT = dict(cos=0x7000, sin=0x7100)
ERRORS = [
    # what the packed form adds
    (dict(cu=None), -1, "null cu_seqlens_"), (dict(total=0), -1, "total_"), (dict(total=-1), -1, "total_"),
    (dict(total=(1 << 28) + 1), -1, "total_"), (dict(max_new=0), -1, "max_seqlen_"), (dict(max_new=-4), -1, "max_seqlen_"),
    (dict(max_new=(1 << 28) + 1), -1, "max_seqlen_"),
    (dict(total=1 << 28, H_kv=4096, H=8192), -1, "2^40"),               # 2^28 * 2 * 2^12 = 2^41 rows of K and V
    (dict(total=1 << 28, H_kv=1, H=8192, **ROT), -1, "2^40"),           # 2^28 * 2^13 rows of Q
    # the fixed append's errors, reached through the packed entry points
    (dict(k_new=None), -1, "null k_new"), (dict(v_new=None), -1, "null v_new"), (dict(lens=None), -1, "null cache_seqlens"),
    (dict(out=None), -1, "null seqlens_out"), (dict(out=0x3000), -1, "seqlens_out must not be cache_seqlens"),
    (dict(k_strides=(-1, 64, 64, 1)), -1, "negative"), (dict(kn_strides=(64, -64, 1)), -1, "negative"),
    (dict(q_strides=(64, 64, -1)), -1, "negative"), (dict(cos_stride=-32, **ROT), -1, "negative"),
    (dict(cos=0x7000), -1, "null rotary_sin"), (dict(sin=0x7100), -1, "null rotary_cos"),
    (dict(rotary_dim=63, **ROT), -1, "rotary_dim"), (dict(rotary_dim=0, **ROT), -1, "rotary_dim"),
    (dict(rotary_dim=66, **ROT), -1, "rotary_dim"), (dict(S_rot=0, **ROT), -1, "S_rot"), (dict(q_rot=None, **ROT), -1, "null q_rot"),
    (dict(K=None), -1, "null K"), (dict(ptr=None), -1, "null V"),
    (dict(table=0x4000, page_size=0), -1, "page_size"), (dict(table=0x4000, max_blocks=0), -1, "max_blocks"),
    (dict(table=0x4000, num_blocks=0), -1, "num_blocks"), (dict(table=0x4000, max_blocks=(1 << 22) + 1), -1, "2^28"),
    (dict(table=0x4000, table_stride=-1), -1, "block_table_stride"),
    (dict(S_k=0), -1, "S_k"), (dict(S_k=(1 << 28) + 1), -1, "S_k"),
    (dict(B=0), -1, "B must"), (dict(B=65536), -1, "B must"), (dict(H_kv=0), -1, "H_kv"), (dict(H=8, H_kv=3), -1, "H_kv"),
    (dict(H=0), -1, "H must"), (dict(null_q_strides=True), -1, "q_strides"),
    (dict(kd=0x3000, kd_strides=(2, 1)), -1, "descale"),
    (dict(kv_dtype=F8E4, kd=0x3000), -1, "k_descale_strides"), (dict(kv_dtype=F8E4, kd=0x3000, kd_strides=(-2, 1)), -1, "negative"),
    (dict(dtype=F8E4), -2, "fp8"), (dict(dtype=F8E5), -2, "fp8"), (dict(dtype=F8E4, kv_dtype=F8E5), -2, " dtype_enum"),
    (dict(dtype=F32, kv_dtype=F8E4), -2, " dtype_enum"), (dict(kv_dtype=F32), -2, "kv_dtype_enum"), (dict(kv_dtype=99), -2, "kv_dtype_enum"),
    (dict(dtype=99), -2, "dtype"), (dict(d=513), -2, "[1, 512]"), (dict(d=0), -2, "[1, 512]"),
]


@pytest.mark.parametrize("kwargs,code,needle", ERRORS)
@pytest.mark.parametrize("call", [_append, _fused])
def test_argument_errors_before_any_launch(call, kwargs, code, needle):
    rc, msg = call(**kwargs)
    assert rc == code, (rc, msg)
    assert needle in msg, msg


def test_the_new_messages_name_the_new_arguments():
    assert "cu_seqlens_new" in _append(cu=None)[1] and "total_new" in _append(total=0)[1]
    assert "max_seqlen_new" in _append(max_new=0)[1] and "total_new * max(H, 2 * H_kv)" in _append(total=1 << 28, H=4096, H_kv=4096)[1]


@pytest.mark.parametrize("kwargs,code,needle", [
    # the packed-query call's own errors come back from the fused call before the append is launched
    (dict(Q=None), -1, "null Q"), (dict(Q=None, **ROT), -1, "null Q"), (dict(num_splits=129), -1, "num_splits"),
    (dict(num_splits=4), -1, "workspace"), (dict(variant=7), -2, "variant"), (dict(variant=2, d=40, rotary_dim=40), -2, "mfma16"),
    (dict(variant=2, table=0x4000, page_size=48), -2, "page_size % 64"), (dict(o_strides=(512, -64, 1)), -1, "negative"),
    (dict(l_stride=-1), -1, "l_head_stride"), (dict(wl=-2), -1, "window"),
])
def test_fused_call_reports_the_attention_errors_before_any_launch(kwargs, code, needle):
    rc, msg = _fused(**kwargs)
    assert rc == code, (rc, msg)
    assert needle in msg, msg


def test_a_null_q_is_the_cache_update_alone():
    """Without Q its arguments are not looked at: H may be anything and does not count towards the row bound (the call then needs a
    device, which a negative stride of an unrelated argument stands in for here, so nothing is launched)."""
    rc, msg = _append(Q=None, q_rot=None, H=0, null_q_strides=True, kn_strides=(-1, 1, 1))
    assert rc == -1 and "negative" in msg
    rc, msg = _append(Q=None, q_rot=None, H=1 << 30, total=1 << 28, H_kv=1, kn_strides=(-1, 1, 1))
    assert rc == -1 and "negative" in msg


BF = torch.bfloat16


def _cpu():
    K = torch.zeros(2, 2, 128, 64, dtype=BF)
    return dict(K=K, V=K, k_new=torch.zeros(5, 2, 64, dtype=BF), v_new=torch.zeros(5, 2, 64, dtype=BF),
                cu=torch.tensor([0, 2, 5], dtype=torch.int32), max_new=3, lens=torch.tensor([3, 50], dtype=torch.int32),
                rotary_cos=torch.zeros(256, 32, dtype=BF), rotary_sin=torch.zeros(256, 32, dtype=BF), Q=torch.zeros(5, 8, 64, dtype=BF))


def _bad_cases():
    b = _cpu()
    kn, cos, K = b["k_new"], b["rotary_cos"], b["K"]
    one = torch.zeros(1, 1, 1, dtype=BF)
    return [
        dict(v_new=None), dict(k_new=None),                                                   # half a pair
        dict(rotary_sin=None), dict(rotary_cos=None),
        dict(k_new=None, v_new=None),                                                         # rotary without k_new
        dict(lens=None),                                                                      # k_new without cache_seqlens
        dict(k_new=kn[0], v_new=kn[0]), dict(k_new=kn[None], v_new=kn[None]), dict(v_new=kn[:4]),   # packed shapes
        dict(k_new=kn[:0], v_new=kn[:0]), dict(k_new=kn[:, :1], v_new=kn[:, :1]), dict(k_new=kn[..., :32], v_new=kn[..., :32]),
        dict(k_new=one.expand((1 << 28) + 1, 2, 64), v_new=one.expand((1 << 28) + 1, 2, 64), Q=None),   # total_new
        dict(k_new=one.expand(1 << 28, 4096, 64), v_new=one.expand(1 << 28, 4096, 64), Q=None,          # the row bound
             K=torch.zeros(1, 1, 1, 1, dtype=BF).expand(2, 4096, 128, 64), V=torch.zeros(1, 1, 1, 1, dtype=BF).expand(2, 4096, 128, 64)),
        dict(k_new="k", v_new="k"),
        dict(cu=b["cu"].long()), dict(cu=b["cu"][:1]), dict(cu=b["cu"].view(1, 3)), dict(cu=torch.zeros(6, dtype=torch.int32)[::2]),
        dict(cu=b["cu"].to("meta")), dict(cu=[0, 2, 5]),
        dict(cu=torch.tensor([0, 2, 4, 5], dtype=torch.int32)),                               # B + 1 entries for the cache's B
        dict(max_new=0), dict(max_new=(1 << 28) + 1), dict(max_new=3.0), dict(max_new=True),
        dict(k_new=kn.float(), v_new=kn.float()), dict(v_new=kn.half()),                      # dtypes
        dict(k_new=kn.to(torch.float8_e5m2), v_new=kn.to(torch.float8_e5m2)),
        dict(k_new=kn.to("meta"), v_new=kn.to("meta")),                                       # device
        dict(lens=b["lens"].long()), dict(lens=b["lens"][:1]),
        dict(rotary_cos=cos.float(), rotary_sin=cos.float()), dict(rotary_sin=cos[:, :16]), dict(rotary_cos=cos[0], rotary_sin=cos[0]),
        dict(rotary_cos=torch.zeros(256, 33, dtype=BF), rotary_sin=torch.zeros(256, 33, dtype=BF)),
        dict(rotary_cos=torch.zeros(256, 64, dtype=BF)[:, ::2]),                              # non-unit last stride
        dict(k_descale=torch.ones(2, 2)),                                                     # descale with a 16-bit cache
        dict(K=K.to(torch.float8_e4m3fn), V=K.to(torch.float8_e4m3fn), k_descale=torch.ones(3, 2)),
        dict(K=K.float(), V=K.float()),                                                       # k_new not in the cache's dtype
        dict(table=torch.zeros(3, 4, dtype=torch.int32), K=torch.zeros(10, 2, 16, 64, dtype=BF), V=torch.zeros(10, 2, 16, 64, dtype=BF)),
    ]


@pytest.mark.parametrize("idx", range(len(_bad_cases())))
def test_check_and_wrapper_raise_value_errors_on_cpu_tensors(idx):
    kw = _bad_cases()[idx]
    a = dict(_cpu(), **kw)
    with pytest.raises(ValueError):
        check_kvcache_append_varlen_args(a["K"], a["V"], a["k_new"], a["v_new"], a["cu"], a["max_new"], a["lens"], a.get("k_descale"), None,
                                         a.get("table"), a["rotary_cos"], a["rotary_sin"])
    with pytest.raises(ValueError):
        fa.kvcache_append_varlen(a["K"], a["V"], a["k_new"], a["v_new"], a["cu"], a["max_new"], a["lens"], k_descale=a.get("k_descale"),
                                 block_table=a.get("table"), rotary_cos=a["rotary_cos"], rotary_sin=a["rotary_sin"])


def test_q_beside_the_packed_tokens():
    a = _cpu()
    args = (a["K"], a["V"], a["k_new"], a["v_new"], a["cu"], a["max_new"], a["lens"], None, None, None, a["rotary_cos"], a["rotary_sin"])
    check_kvcache_append_varlen_args(*args, a["Q"])
    for Q in (a["Q"][:4], a["Q"][..., :32], a["Q"][0], a["Q"].half(), "q"):
        with pytest.raises(ValueError):
            check_kvcache_append_varlen_args(*args, Q)
    wide = torch.zeros(1, 1, 1, dtype=BF)
    with pytest.raises(ValueError, match="2\\^40"):  # Q's heads count towards the row bound
        check_kvcache_append_varlen_args(a["K"], a["V"], wide.expand(1 << 28, 2, 64), wide.expand(1 << 28, 2, 64), a["cu"], 3, a["lens"],
                                         Q=wide.expand(1 << 28, 8192, 64))


def _forward(a, **kw):
    return fa.flash_attention_varlen_kvcache_forward(a["Q"], a["K"], a["V"], a["cu"], a["max_new"], a["lens"], "cpu", num_splits=1,
                                                     k_descale=a.get("k_descale"), block_table=a.get("table"), **kw)


# (the cases that set Q are the append-only call's: total_q is Q's here)
@pytest.mark.parametrize("idx", [i for i, kw in enumerate(_bad_cases()) if "Q" not in kw])
def test_the_new_keywords_of_the_packed_query_call_raise_on_cpu_tensors(idx):
    a = dict(_cpu(), **_bad_cases()[idx])
    if a["K"].dtype == torch.float32:
        a["Q"] = a["Q"].float()  # Q follows the cache: the error left is k_new's dtype
    with pytest.raises(ValueError):
        _forward(a, k_new=a["k_new"], v_new=a["v_new"], rotary_cos=a["rotary_cos"], rotary_sin=a["rotary_sin"])


def test_new_keywords_shape_and_device_against_q():
    a = _cpu()
    kn = a["k_new"]
    six = torch.zeros(6, 2, 64, dtype=BF)
    for k in (six, kn.float(), kn.half()):  # total_q, Q's dtype
        with pytest.raises(ValueError):
            _forward(a, k_new=k, v_new=k)
    with pytest.raises(ValueError):  # rotary tables without k_new, as in the fixed call
        _forward(a, rotary_cos=a["rotary_cos"], rotary_sin=a["rotary_sin"])
    with pytest.raises(ValueError):
        _forward(dict(a, lens=None), k_new=kn, v_new=kn)
    with pytest.raises(ValueError):
        fa.kvcache_append_varlen(a["K"], a["V"], None, None, a["cu"], 3, a["lens"])


def test_what_is_fine_reaches_the_launch():
    """... which refuses CPU tensors."""
    a = _cpu()
    k8 = a["K"].to(torch.float8_e5m2)
    pool, table = torch.zeros(10, 2, 16, 64, dtype=BF), torch.zeros(2, 4, dtype=torch.int32)
    wide = torch.zeros(5, 3, 72, dtype=BF)[:, :2, :64]
    cos = a["rotary_cos"]
    for kw in (dict(), dict(rotary_cos=None, rotary_sin=None), dict(K=k8, V=k8, k_descale=torch.ones(2, 2)), dict(k_new=wide, v_new=wide),
               dict(K=pool, V=pool, table=table), dict(rotary_cos=cos[:, :8], rotary_sin=cos[:, :8]),
               dict(cu=torch.tensor([0, 0, 9], dtype=torch.int32)), dict(max_new=1)):
        b = dict(a, **kw)
        with pytest.raises(NotImplementedError):
            _forward(b, k_new=b["k_new"], v_new=b["v_new"], rotary_cos=b["rotary_cos"], rotary_sin=b["rotary_sin"])
        with pytest.raises(NotImplementedError):
            fa.kvcache_append_varlen(b["K"], b["V"], b["k_new"], b["v_new"], b["cu"], b["max_new"], b["lens"], k_descale=b.get("k_descale"),
                                     block_table=b.get("table"), rotary_cos=b["rotary_cos"], rotary_sin=b["rotary_sin"])


def test_keyword_free_calls_of_check_varlen_kvcache_args_behave_as_before():
    a = _cpu()
    assert check_varlen_kvcache_args(a["Q"], a["K"], a["V"], a["cu"], 3, a["lens"], None, 0) is None
    assert check_varlen_kvcache_args(a["Q"], a["K"], a["V"], a["cu"], 3, None, (4, 0), 2) is None  # cache_seqlens stays optional
    for bad in (dict(Q=a["Q"][0]), dict(cu=a["cu"].long()), dict(max_q=0), dict(lens=a["lens"][:1]), dict(window=(-2, 0)), dict(n=129),
                dict(K=a["K"].float())):
        b = dict(dict(Q=a["Q"], K=a["K"], cu=a["cu"], max_q=3, lens=a["lens"], window=None, n=0), **bad)
        with pytest.raises(ValueError):
            check_varlen_kvcache_args(b["Q"], b["K"], b["K"], b["cu"], b["max_q"], b["lens"], b["window"], b["n"])
    with pytest.raises(NotImplementedError):  # and the call without the keywords still reaches the existing launch
        _forward(a)
