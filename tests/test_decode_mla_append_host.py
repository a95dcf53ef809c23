"""The latent-cache append (fa2_kvcache_mla_append, fa2_kvcache_mla_append_varlen, fa2_fwd_kvcache_mla_append), the part that needs
no GPU: the exported symbols, every argument error before any launch (fake pointers), the Python wrappers' errors on CPU tensors,
and the restatement the GPU tests use against the one of the ordinary append."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from conftest import ROOT

import flash_attention_dlrs_amd as fa
from flash_attention_dlrs_amd import _lib
from decode_append_restatement import bits, expected_append
from mla_append_restatement import expected_mla_append, expected_mla_append_packed

F8E4, F8E5, F32, BF16 = _lib.FA2_DTYPE_F8E4M3, _lib.FA2_DTYPE_F8E5M2, _lib.FA2_DTYPE_F32, _lib.FA2_DTYPE_BF16
NEW = ("fa2_kvcache_mla_append", "fa2_kvcache_mla_append_varlen", "fa2_fwd_kvcache_mla_append")


def test_symbols_exported_declared_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fa2_fwd.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exports = open(os.path.join(ROOT, "flash_attention_dlrs_amd", "csrc", "fa2_exports.map")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS
        assert re.search(rf"\b{name}\s*\(", header), name
        assert re.search(rf"\bT {name}\b", out), name
        assert re.search(rf"\b{name};", exports), name
        assert callable(getattr(_lib, name)) and getattr(_lib.lib(), name) is not None
    for name in ("mla_kvcache_append", "mla_kvcache_append_varlen", "check_mla_append_args"):
        assert name in fa.__all__ and callable(getattr(fa, name))


def _i64(v):
    return None if v is None else (ctypes.c_int64 * len(v))(*v)


def _args(KV=0x1000, c_new=0x2000, pe_new=0x2800, lens=0x3000, out=0x3100, table=None, table_stride=8, B=2, H=16, H_kv=1, N_q=1,
          N_new=1, S_k=256, num_blocks=32, page_size=64, max_blocks=8, d=576, d_v=512, dtype=BF16, kv_dtype=None, kd=None,
          kd_strides=None, cos=None, sin=None, cos_stride=32, S_rot=512, rotary_dim=64, Q=0x5000, q_rot=0x6000, kv_strides=None,
          cn_strides=None, pn_strides=None, q_strides=None, num_splits=1, variant=0, cu=0x3200, total_new=2, max_new=1, ptr=0x7000):
    return dict(locals())


def _strides(a, packed=False):
    d, d_v, n = a["d"], a["d_v"], a["N_new"]
    ks = a["kv_strides"] or (a["H_kv"] * 256 * d, 256 * d, d, 1)
    if packed:
        cn = a["cn_strides"] or (a["H_kv"] * d_v, d_v, 1)
        pn = a["pn_strides"] or (a["H_kv"] * (d - d_v), d - d_v, 1)
        qs = a["q_strides"] or (a["H"] * d, d, 1)
    else:
        cn = a["cn_strides"] or (a["H_kv"] * n * d_v, n * d_v, d_v, 1)
        pn = a["pn_strides"] or (a["H_kv"] * n * (d - d_v), n * (d - d_v), d - d_v, 1)
        qs = a["q_strides"] or (a["H"] * a["N_q"] * d, a["N_q"] * d, d, 1)
    return _i64(ks), _i64(cn), _i64(pn), _i64(qs), a["dtype"] if a["kv_dtype"] is None else a["kv_dtype"]


def _append(**kw):
    a = _args(**kw)
    ks, cn, pn, qs, kv = _strides(a)
    rc = _lib.lib().fa2_kvcache_mla_append(a["KV"], ks, a["table"], a["table_stride"], a["c_new"], a["pe_new"], cn, pn, a["lens"],
                                           a["out"], a["kd"], _i64(a["kd_strides"]), a["cos"], a["sin"], a["cos_stride"],
                                           a["cos_stride"], a["S_rot"], a["rotary_dim"], 0, a["Q"], a["q_rot"], qs, a["H"], a["N_q"],
                                           0, a["B"], a["H_kv"], a["N_new"], a["S_k"], a["num_blocks"], a["page_size"],
                                           a["max_blocks"], a["d"], a["d_v"], a["dtype"], kv, None)
    return rc, _lib.lib().fa2_last_error().decode()


def _packed(**kw):
    a = _args(**kw)
    ks, cn, pn, qs, kv = _strides(a, packed=True)
    rc = _lib.lib().fa2_kvcache_mla_append_varlen(a["KV"], ks, a["table"], a["table_stride"], a["c_new"], a["pe_new"], cn, pn, a["cu"],
                                                  a["lens"], a["out"], a["kd"], _i64(a["kd_strides"]), a["cos"], a["sin"],
                                                  a["cos_stride"], a["cos_stride"], a["S_rot"], a["rotary_dim"], 0, a["Q"],
                                                  a["q_rot"], qs, a["H"], 0, a["B"], a["H_kv"], a["total_new"], a["max_new"],
                                                  a["S_k"], a["num_blocks"], a["page_size"], a["max_blocks"], a["d"], a["d_v"],
                                                  a["dtype"], kv, None)
    return rc, _lib.lib().fa2_last_error().decode()


def _fused(**kw):
    a = _args(**kw)
    ks, cn, pn, qs, kv = _strides(a)
    os_ = _i64((a["H"] * a["N_q"] * a["d_v"], a["N_q"] * a["d_v"], a["d_v"], 1))
    rc = _lib.lib().fa2_fwd_kvcache_mla_append(a["Q"], a["KV"], a["ptr"], a["ptr"], qs, ks, os_, _i64((a["H"] * a["N_q"], a["N_q"])),
                                               a["lens"], a["out"], a["table"], a["table_stride"], a["kd"], _i64(a["kd_strides"]),
                                               a["c_new"], a["pe_new"], cn, pn, a["cos"], a["sin"], a["cos_stride"], a["cos_stride"],
                                               a["S_rot"], a["rotary_dim"], 0, a["q_rot"], a["B"], a["H"], a["H_kv"], a["N_q"],
                                               a["N_new"], a["S_k"], a["num_blocks"], a["page_size"], a["max_blocks"], a["d"],
                                               a["d_v"], a["dtype"], kv, 0, 1.0, -1, -1, a["num_splits"], None, 0, a["variant"], None)
    return rc, _lib.lib().fa2_last_error().decode()


ROT = dict(cos=0x7000, sin=0x7100)
ERRORS = [
    # the head sizes and the rotary range behind d_v
    (dict(d=577), -2, "[2, 576]"), (dict(d=1, d_v=1), -2, "[2, 576]"), (dict(d_v=0), -2, "d_v"), (dict(d_v=576), -2, "d_v"),
    (dict(d=64, d_v=64), -2, "d_v"),
    (dict(rotary_dim=66, **ROT), -1, "rotary_dim"), (dict(rotary_dim=63, **ROT), -1, "rotary_dim"), (dict(rotary_dim=0, **ROT), -1, "rotary_dim"),
    (dict(rotary_dim=64, d_v=544, **ROT), -1, "d - d_v"), (dict(rotary_dim=1, **ROT), -1, "rotary_dim"),
    (dict(cos=0x7000), -1, "null rotary_sin"), (dict(sin=0x7100), -1, "null rotary_cos"), (dict(S_rot=0, **ROT), -1, "S_rot"),
    (dict(cos_stride=-32, **ROT), -1, "negative"), (dict(q_rot=None, **ROT), -1, "null q_rot"),
    # null pointers, by their names here
    (dict(KV=None), -1, "null KV"), (dict(c_new=None), -1, "null c_new"), (dict(pe_new=None), -1, "null pe_new"),
    (dict(lens=None), -1, "null cache_seqlens"), (dict(out=None), -1, "null seqlens_out"),
    (dict(out=0x3000), -1, "seqlens_out must not be cache_seqlens"),
    # strides
    (dict(kv_strides=(-1, 576, 576, 1)), -1, "kv_strides"),
    # the cache's sizes
    (dict(table=0x4000, page_size=0), -1, "page_size"), (dict(table=0x4000, max_blocks=0), -1, "max_blocks"),
    (dict(table=0x4000, num_blocks=0), -1, "num_blocks"), (dict(table=0x4000, max_blocks=(1 << 22) + 1), -1, "2^28"),
    (dict(table=0x4000, table_stride=-1), -1, "block_table_stride"), (dict(S_k=0), -1, "S_k"), (dict(S_k=(1 << 28) + 1), -1, "S_k"),
    (dict(B=0), -1, "B must"), (dict(B=65536), -1, "B must"), (dict(H_kv=0), -1, "H_kv"), (dict(H=16, H_kv=3), -1, "H_kv"),
    (dict(H=0), -1, "H must"),
    # the one descale
    (dict(kd=0x3000, kd_strides=(1, 1)), -1, "kv_descale"),                               # with a cache in the inputs' dtype
    (dict(kv_dtype=F8E4, kd=0x3000), -1, "kv_descale_strides"), (dict(kv_dtype=F8E4, kd=0x3000, kd_strides=(-1, 1)), -1, "kv_descale_strides"),
    # dtype combinations
    (dict(dtype=F8E4), -2, "fp8"), (dict(dtype=F8E5), -2, "fp8"), (dict(dtype=F32, kv_dtype=F8E4), -2, " dtype_enum"),
    (dict(kv_dtype=F32), -2, "kv_dtype_enum"), (dict(kv_dtype=99), -2, "kv_dtype_enum"), (dict(dtype=99), -2, "dtype"),
]
FIXED_ONLY = [(dict(q_strides=(576, 576, 576, -1)), -1, "q_strides"), (dict(N_new=0), -1, "N_new"), (dict(N_new=(1 << 28) + 1), -1, "N_new"), (dict(N_q=0), -1, "N_q"),
              (dict(cn_strides=(512, 512, -512, 1)), -1, "c_new_strides"), (dict(pn_strides=(64, 64, 64, -1)), -1, "pe_new_strides")]
PACKED_ONLY = [(dict(q_strides=(576, 576, -1)), -1, "q_strides"), (dict(cu=None), -1, "null cu_seqlens_new"), (dict(total_new=0), -1, "total_new"), (dict(total_new=(1 << 28) + 1), -1, "total_new"),
               (dict(max_new=0), -1, "max_seqlen_new"), (dict(max_new=(1 << 28) + 1), -1, "max_seqlen_new"),
               (dict(cn_strides=(-512, 512, 1)), -1, "c_new_strides"), (dict(pn_strides=(64, 64, -1)), -1, "pe_new_strides")]


@pytest.mark.parametrize("call,kwargs,code,needle", [(c, *e) for c in (_append, _packed, _fused) for e in ERRORS]
                         + [(c, *e) for c in (_append, _fused) for e in FIXED_ONLY] + [(_packed, *e) for e in PACKED_ONLY])
def test_argument_errors_before_any_launch(call, kwargs, code, needle):
    rc, msg = call(**kwargs)
    assert rc == code, (rc, msg)
    assert needle in msg, msg


@pytest.mark.parametrize("kwargs,code,needle", [
    # the decode call's own errors come back from the fused call before the append is launched
    (dict(Q=None), -1, "null Q"), (dict(ptr=None), -1, "null O"), (dict(num_splits=129), -1, "num_splits"),
    (dict(num_splits=4), -1, "workspace"), (dict(variant=7), -2, "variant"), (dict(variant=2), -2, "variant"),
    (dict(variant=3, d=192, d_v=128), -2, "d = 576"), (dict(variant=3, table=0x4000, page_size=16), -2, "page_size % 64"),
    (dict(variant=3, KV=0x1004), -2, "16-byte"), (dict(Q=None, **ROT), -1, "null Q"),
])
def test_fused_call_reports_the_decode_errors_before_any_launch(kwargs, code, needle):
    rc, msg = _fused(**kwargs)
    assert rc == code, (rc, msg)
    assert needle in msg, msg


def test_a_null_q_is_the_cache_update_alone():
    """Without Q its arguments are not looked at: the call gets past every check up to the strides (a negative one of c_new stands
    in for the device a launch would need, so nothing is launched)."""
    for call, bad in ((_append, dict(cn_strides=(-1, 1, 1, 1))), (_packed, dict(cn_strides=(-1, 1, 1)))):
        rc, msg = call(Q=None, q_rot=None, H=0, N_q=0, q_strides=(-1, -1, -1, -1)[:len(bad["cn_strides"])], **bad)
        assert rc == -1 and "negative" in msg


BF = torch.bfloat16


def _cpu_case():
    KV = torch.zeros(2, 1, 128, 576, dtype=BF)
    new = torch.zeros(2, 1, 3, 576, dtype=BF)
    return dict(KV=KV, kv_new=new, lens=torch.tensor([3, 50], dtype=torch.int32), d_v=512, cos=torch.zeros(256, 32, dtype=BF),
                sin=torch.zeros(256, 32, dtype=BF), Q=torch.zeros(2, 16, 1, 576, dtype=BF))


def _py_calls(a):
    """the three fixed-form entry points on one set of arguments"""
    kw = dict(d_v=a["d_v"], kv_descale=a.get("kv_descale"), block_table=a.get("table"), rotary_cos=a["cos"], rotary_sin=a["sin"])
    yield lambda: fa.check_mla_append_args(a["KV"], a["kv_new"], a["lens"], a["d_v"], a.get("kv_descale"), a.get("table"), a["cos"], a["sin"])
    yield lambda: fa.mla_kvcache_append(a["KV"], a["kv_new"], a["lens"], **kw)
    yield lambda: fa.flash_attention_mla_decode_forward(a["Q"], a["KV"], a["lens"], "cpu", num_splits=1, kv_new=a["kv_new"], **kw)


def test_python_wrappers_raise_value_errors_on_cpu_tensors():
    base = _cpu_case()
    new, cos, KV = base["kv_new"], base["cos"], base["KV"]
    pool, table = torch.zeros(9, 1, 64, 576, dtype=BF), torch.zeros(2, 4, dtype=torch.int32)
    bad = [
        dict(kv_new=(new[..., :512], new[..., :32])), dict(kv_new=(new[..., :500], new[..., 512:])),   # widths that do not add up to d
        dict(kv_new=new[..., :512]), dict(kv_new=(new, new)), dict(kv_new=(new[..., :512],)), dict(kv_new="x"),
        dict(kv_new=(new[:, :, :2, :512], new[..., 512:])), dict(kv_new=new[0]), dict(kv_new=new[:1]), dict(kv_new=new[:, :, :0]),
        dict(kv_new=new.expand(2, 2, 3, 576)),                                                            # H_kv
        dict(d_v=0), dict(d_v=576), dict(d_v=512.0), dict(d_v=True),                                       # d_v out of range
        dict(d_v=544),                                                                                    # rotary_dim > d - d_v
        dict(cos=torch.zeros(256, 33, dtype=BF), sin=torch.zeros(256, 33, dtype=BF)),
        dict(cos=cos.float(), sin=cos.float()), dict(sin=cos[:, :16]), dict(cos=cos[0], sin=cos[0]),       # the tables
        dict(cos=torch.zeros(256, 64, dtype=BF)[:, ::2]), dict(cos=cos.to("meta"), sin=cos.to("meta")),
        dict(cos=None), dict(sin=None), dict(cos=cos[:0], sin=cos[:0]),
        dict(kv_descale=torch.ones(2, 1)),                                                                # with a 16-bit cache
        dict(KV=KV.to(torch.float8_e4m3fn), kv_descale=torch.ones(3, 1)),
        dict(KV=KV.to(torch.float8_e4m3fn), kv_descale=torch.ones(2, 1, dtype=torch.float64)),
        dict(kv_new=new.to(torch.float8_e5m2), KV=KV.to(torch.float8_e5m2)),                              # fp8 kv_new
        dict(kv_new=new.float()), dict(kv_new=(new[..., :512], new[..., 512:].half())),                    # dtypes
        dict(kv_new=new.to("meta")),                                                                      # device
        dict(lens=None), dict(lens=base["lens"].long()), dict(lens=base["lens"][:1]),                      # kv_new without cache_seqlens
        dict(KV=pool, table=torch.zeros(3, 4, dtype=torch.int32)), dict(KV=pool, table=table.long()),
        dict(KV=pool, table=torch.zeros(2, 8, dtype=torch.int32)[:, ::2]), dict(KV=pool, table=table.to("meta")),
        dict(KV=torch.zeros(2, 1, 128, 600, dtype=BF), kv_new=torch.zeros(2, 1, 3, 600, dtype=BF), Q=torch.zeros(2, 16, 1, 600, dtype=BF)),
    ]
    for kw in bad:
        a = dict(base, **kw)
        for call in _py_calls(a):
            with pytest.raises(ValueError):
                call()
    with pytest.raises(ValueError):
        fa.mla_kvcache_append(KV, None, base["lens"])
    # rotary tables without kv_new
    with pytest.raises(ValueError, match="kv_new"):
        fa.flash_attention_mla_decode_forward(base["Q"], KV, base["lens"], "cpu", rotary_cos=cos, rotary_sin=cos)
    with pytest.raises(ValueError):
        fa.flash_attention_mla_decode_forward(base["Q"], KV, base["lens"], "cpu", rotary_sin=cos)
    # Q beside kv_new
    for Q in (base["Q"].half(), base["Q"][..., :512], base["Q"][:1]):
        with pytest.raises(ValueError):
            fa.flash_attention_mla_decode_forward(Q, KV, base["lens"], "cpu", kv_new=new)
    # what is fine reaches the launch, which refuses CPU tensors
    k8 = KV.to(torch.float8_e5m2)
    nhd = torch.zeros(2, 3, 1, 576, dtype=BF).transpose(1, 2)
    for kw in (dict(), dict(cos=None, sin=None), dict(kv_new=(new[..., :512].clone(), new[..., 512:].clone())), dict(kv_new=nhd),
               dict(KV=k8, kv_descale=torch.ones(2, 1)), dict(KV=k8, kv_descale=torch.ones(1)), dict(KV=pool, table=table),
               dict(cos=cos[:, :8], sin=cos[:, :8]), dict(kv_new=[new[..., :512], torch.zeros(2, 1, 3, 128, dtype=BF)[..., ::2]]),
               dict(KV=KV[..., :192], kv_new=new[..., :192], Q=base["Q"][..., :192], d_v=128)):
        a = dict(base, **kw)
        calls = list(_py_calls(a))
        calls[0]()  # the pure check takes them
        for call in calls[1:]:
            with pytest.raises(NotImplementedError):
                call()


def test_packed_wrapper_errors():
    base = _cpu_case()
    KV, cos = base["KV"], base["cos"]
    new = torch.zeros(6, 1, 576, dtype=BF)
    cu = torch.tensor([0, 2, 6], dtype=torch.int32)
    call = lambda **kw: fa.mla_kvcache_append_varlen(kw.pop("KV", KV), kw.pop("kv_new", new), kw.pop("cu", cu), kw.pop("max_new", 4),
                                                     kw.pop("lens", base["lens"]), rotary_cos=cos, rotary_sin=cos, **kw)
    for kw in (dict(cu=cu.long()), dict(cu=cu[:1]), dict(cu=None), dict(cu=torch.zeros(2, 2, dtype=torch.int32)), dict(cu=cu.to("meta")),
               dict(cu=torch.tensor([0, 1, 2, 3, 4, 6], dtype=torch.int32)[::2]),
               dict(max_new=0), dict(max_new=None), dict(max_new=2.0), dict(max_new=True), dict(max_new=(1 << 28) + 1),
               dict(kv_new=new[None]), dict(kv_new=new[:0]), dict(kv_new=(new[..., :512], new[:5, :, 512:])), dict(kv_new=None),
               dict(lens=torch.zeros(3, dtype=torch.int32)), dict(d_v=544), dict(kv_descale=torch.ones(2, 1))):
        with pytest.raises(ValueError):
            call(**kw)
    for kw in (dict(), dict(kv_new=(new[..., :512], new[..., 512:].clone())), dict(max_new=1),
               dict(KV=KV.to(torch.float8_e4m3fn), kv_descale=torch.ones(2, 1))):
        with pytest.raises(NotImplementedError):
            call(**kw)


def test_general_call_still_refuses_the_append_with_d_v_not_d():
    a = _cpu_case()
    for kw, needle in ((dict(k_new=a["kv_new"], v_new=a["kv_new"][..., :512]), "k_new"), (dict(rotary_cos=a["cos"], rotary_sin=a["sin"]), "rotary_cos")):
        with pytest.raises(ValueError, match=f"{needle} is not supported with d_v != d"):
            fa.flash_attention_kvcache_forward(a["Q"], a["KV"], a["KV"][..., :512], a["lens"], "cpu", **kw)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_restatement_agrees_with_the_ordinary_appends(dtype):
    """Without rotary and with a cache in the inputs' dtype the latent row is k_new's two halves: expected_append's K."""
    g = torch.Generator().manual_seed(7)
    B, H_kv, S, d, n = 3, 2, 40, 64, 3
    K0 = torch.randn(B, H_kv, S, d, generator=g).to(dtype)
    k_new = torch.randn(B, H_kv, n, d, generator=g).to(dtype)
    lens = torch.tensor([-2, 17, 38], dtype=torch.int32)
    K, _, start, out = expected_append(K0, K0, k_new, k_new, lens)
    KV, start2, out2 = expected_mla_append(K0, k_new[..., :32], k_new[..., 32:], lens, 32)
    assert torch.equal(bits(KV), bits(K)) and torch.equal(start, start2) and torch.equal(out, out2)
    assert not torch.equal(bits(KV), bits(K0))
    # ... through a table, and the packed form on the same tokens
    pool0 = torch.randn(7, H_kv, 16, d, generator=g).to(dtype)
    table = torch.tensor([[0, 1, 1], [2, 3, 1], [4, 5, 99]], dtype=torch.int32)
    lens = torch.tensor([0, 15, 46], dtype=torch.int32)
    K, _, _, out = expected_append(pool0, pool0, k_new, k_new, lens, table)
    KV, _, out2 = expected_mla_append(pool0, k_new[..., :32], k_new[..., 32:], lens, 32, table)
    assert torch.equal(bits(KV), bits(K)) and torch.equal(out, out2)
    packed = k_new.permute(0, 2, 1, 3).reshape(B * n, H_kv, d)
    KVp, outp = expected_mla_append_packed(pool0, packed[..., :32], packed[..., 32:], torch.tensor([0, 3, 6, 9], dtype=torch.int32), 3, lens,
                                           32, table)
    assert torch.equal(bits(KVp), bits(K)) and torch.equal(outp, out)
