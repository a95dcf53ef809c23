"""The KV-cache append (fa2_kvcache_append, fa2_fwd_kvcache_append), the part that needs no GPU: the exported symbols, every
argument error before any launch (fake pointers), the Python wrappers' errors on CPU tensors, apply_rotary against an fp64 complex
multiplication, and the restatement of seqlens_out the GPU tests use."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from conftest import ROOT

import flash_attention_dlrs_amd as fa
from flash_attention_dlrs_amd import _lib
from decode_append_restatement import bits, expected_append, new_lengths

F8E4, F8E5, F32, BF16 = _lib.FA2_DTYPE_F8E4M3, _lib.FA2_DTYPE_F8E5M2, _lib.FA2_DTYPE_F32, _lib.FA2_DTYPE_BF16


def test_symbols_exported_declared_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fa2_fwd.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exports = open(os.path.join(ROOT, "flash_attention_dlrs_amd", "csrc", "fa2_exports.map")).read()
    for name in ("fa2_kvcache_append", "fa2_fwd_kvcache_append"):
        assert name in _lib.SYMBOLS
        assert re.search(rf"\b{name}\s*\(", header)
        assert re.search(rf"\bT {name}\b", out)
        assert re.search(rf"\b{name};", exports)
        assert callable(getattr(_lib, name)) and getattr(_lib.lib(), name) is not None
    assert "kvcache_append" in fa.__all__ and "apply_rotary" in fa.__all__


def _i64(v):
    return None if v is None else (ctypes.c_int64 * len(v))(*v)


def _args(ptr=0x1000, K=0x1000, k_new=0x2000, v_new=0x2000, lens=0x3000, out=0x3100, table=None, table_stride=8, B=2, H=8, H_kv=2,
          N_q=1, N_new=1, S_k=256, num_blocks=32, page_size=64, max_blocks=8, d=64, dtype=BF16, kv_dtype=None, kd=None,
          kd_strides=None, cos=None, sin=None, cos_stride=32, S_rot=512, rotary_dim=64, Q=0x5000, q_rot=0x6000, k_strides=None,
          kn_strides=None, q_strides=None, num_splits=1, variant=0):
    return dict(locals())


def _append(**kw):
    a = _args(**kw)
    ks = a["k_strides"] or (a["H_kv"] * 256 * a["d"], 256 * a["d"], a["d"], 1)
    ns = a["kn_strides"] or (a["H_kv"] * a["N_new"] * a["d"], a["N_new"] * a["d"], a["d"], 1)
    qs = a["q_strides"] or (a["H"] * a["N_q"] * a["d"], a["N_q"] * a["d"], a["d"], 1)
    kv = a["dtype"] if a["kv_dtype"] is None else a["kv_dtype"]
    rc = _lib.lib().fa2_kvcache_append(a["K"], a["ptr"], _i64(ks), _i64(ks), a["table"], a["table_stride"], a["k_new"], a["v_new"],
                                       _i64(ns), _i64(ns), a["lens"], a["out"], a["kd"], None, _i64(a["kd_strides"]), None, a["cos"],
                                       a["sin"], a["cos_stride"], a["cos_stride"], a["S_rot"], a["rotary_dim"], 0, a["Q"], a["q_rot"],
                                       _i64(qs), a["H"], a["N_q"], 0, a["B"], a["H_kv"], a["N_new"], a["S_k"], a["num_blocks"],
                                       a["page_size"], a["max_blocks"], a["d"], a["dtype"], kv, None)
    return rc, _lib.lib().fa2_last_error().decode()


def _fused(**kw):
    a = _args(**kw)
    ks = a["k_strides"] or (a["H_kv"] * 256 * a["d"], 256 * a["d"], a["d"], 1)
    ns = a["kn_strides"] or (a["H_kv"] * a["N_new"] * a["d"], a["N_new"] * a["d"], a["d"], 1)
    qs = a["q_strides"] or (a["H"] * a["N_q"] * a["d"], a["N_q"] * a["d"], a["d"], 1)
    kv = a["dtype"] if a["kv_dtype"] is None else a["kv_dtype"]
    rc = _lib.lib().fa2_fwd_kvcache_append(a["Q"], a["K"], a["ptr"], a["ptr"], a["ptr"], _i64(qs), _i64(ks), _i64(ks), _i64(qs),
                                           _i64((a["H"] * a["N_q"], a["N_q"])), a["lens"], a["out"], a["table"], a["table_stride"],
                                           a["kd"], None, _i64(a["kd_strides"]), None, a["k_new"], a["v_new"], _i64(ns), _i64(ns),
                                           a["cos"], a["sin"], a["cos_stride"], a["cos_stride"], a["S_rot"], a["rotary_dim"], 0,
                                           a["q_rot"], a["B"], a["H"], a["H_kv"], a["N_q"], a["N_new"], a["S_k"], a["num_blocks"],
                                           a["page_size"], a["max_blocks"], a["d"], a["dtype"], kv, 0, 1.0, -1, -1, a["num_splits"],
                                           None, 0, a["variant"], None)
    return rc, _lib.lib().fa2_last_error().decode()


ROT = dict(cos=0x7000, sin=0x7100)
ERRORS = [
    # what the issue lists
    (dict(k_new=None), -1, "null k_new"), (dict(v_new=None), -1, "null v_new"), (dict(lens=None), -1, "null cache_seqlens"),
    (dict(out=None), -1, "null seqlens_out"), (dict(out=0x3000), -1, "seqlens_out must not be cache_seqlens"),
    (dict(N_new=0), -1, "N_new"), (dict(N_new=-1), -1, "N_new"), (dict(N_new=(1 << 28) + 1), -1, "N_new"),
    (dict(k_strides=(-1, 64, 64, 1)), -1, "negative"), (dict(kn_strides=(64, 64, -64, 1)), -1, "negative"),
    (dict(q_strides=(64, 64, 64, -1)), -1, "negative"), (dict(cos_stride=-32, **ROT), -1, "negative"),
    (dict(cos=0x7000), -1, "null rotary_sin"), (dict(sin=0x7100), -1, "null rotary_cos"),
    (dict(rotary_dim=63, **ROT), -1, "rotary_dim"), (dict(rotary_dim=0, **ROT), -1, "rotary_dim"),
    (dict(rotary_dim=1, **ROT), -1, "rotary_dim"), (dict(rotary_dim=66, **ROT), -1, "rotary_dim"),
    (dict(S_rot=0, **ROT), -1, "S_rot"), (dict(q_rot=None, **ROT), -1, "null q_rot"),
    # every error of the paged call that still applies
    (dict(K=None), -1, "null K"), (dict(ptr=None), -1, "null V"),
    (dict(table=0x4000, page_size=0), -1, "page_size"), (dict(table=0x4000, max_blocks=0), -1, "max_blocks"),
    (dict(table=0x4000, num_blocks=0), -1, "num_blocks"), (dict(table=0x4000, max_blocks=(1 << 22) + 1), -1, "2^28"),
    (dict(table=0x4000, max_blocks=1 << 30, page_size=1 << 30), -1, "2^28"),
    (dict(table=0x4000, table_stride=-1), -1, "block_table_stride"),
    (dict(S_k=0), -1, "S_k"), (dict(S_k=(1 << 28) + 1), -1, "S_k"),
    (dict(B=0), -1, "B must"), (dict(B=65536), -1, "B must"), (dict(H_kv=0), -1, "H_kv"), (dict(H=8, H_kv=3), -1, "H_kv"),
    (dict(H=0), -1, "H must"), (dict(N_q=0), -1, "N_q"),
    (dict(kd=0x3000, kd_strides=(2, 1)), -1, "descale"),  # descales with a cache in the inputs' dtype
    (dict(kv_dtype=F8E4, kd=0x3000), -1, "k_descale_strides"), (dict(kv_dtype=F8E4, kd=0x3000, kd_strides=(-2, 1)), -1, "negative"),
    # dtype combinations, as in the fp8 call
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


@pytest.mark.parametrize("kwargs,code,needle", [
    # the decode call's own errors come back from the fused call before the append is launched
    (dict(Q=None), -1, "null Q"), (dict(num_splits=129), -1, "num_splits"), (dict(num_splits=4), -1, "workspace"),
    (dict(variant=7), -2, "variant"), (dict(variant=2, d=40, rotary_dim=40), -2, "mfma16"),
    (dict(variant=2, table=0x4000, page_size=48), -2, "page_size % 64"),
    (dict(Q=None, **ROT), -1, "null Q"),
])
def test_fused_call_reports_the_decode_errors_before_any_launch(kwargs, code, needle):
    rc, msg = _fused(**kwargs)
    assert rc == code, (rc, msg)
    assert needle in msg, msg


def test_a_null_q_is_the_cache_update_alone():
    """Without Q its arguments are not looked at: the call gets past every check (and then needs a device, which a negative stride
    of an unrelated argument stands in for here, so nothing is launched)."""
    rc, msg = _append(Q=None, q_rot=None, H=0, N_q=0, q_strides=(-1, -1, -1, -1), kn_strides=(-1, 1, 1, 1))
    assert rc == -1 and "negative" in msg


def test_python_wrappers_raise_value_errors_on_cpu_tensors():
    bf = torch.bfloat16
    Q = torch.zeros(2, 8, 1, 64, dtype=bf)
    K = torch.zeros(2, 2, 128, 64, dtype=bf)
    kn = torch.zeros(2, 2, 3, 64, dtype=bf)
    cos = torch.zeros(256, 32, dtype=bf)
    lens = torch.tensor([3, 50], dtype=torch.int32)
    pool, table = torch.zeros(10, 2, 16, 64, dtype=bf), torch.zeros(2, 4, dtype=torch.int32)
    base = dict(Q=Q, K=K, V=K, lens=lens, k_new=kn, v_new=kn, rotary_cos=cos, rotary_sin=cos)
    bad = [
        dict(v_new=None), dict(k_new=None),                                       # half a pair
        dict(rotary_sin=None), dict(rotary_cos=None),
        dict(k_new=None, v_new=None),                                             # rotary without k_new
        dict(lens=None),                                                          # k_new without cache_seqlens
        dict(k_new=kn[0], v_new=kn[0]), dict(v_new=kn[:, :, :2]),                 # shapes
        dict(k_new=kn[:, :1], v_new=kn[:, :1]), dict(k_new=kn[..., :32], v_new=kn[..., :32]),
        dict(k_new=kn[:1], v_new=kn[:1]), dict(k_new=kn[:, :, :0], v_new=kn[:, :, :0]),
        dict(k_new=kn.float(), v_new=kn.float()), dict(v_new=kn.half()),          # dtypes
        dict(k_new=kn.to("meta"), v_new=kn.to("meta")),                           # device
        dict(rotary_cos=cos.float(), rotary_sin=cos.float()), dict(rotary_sin=cos[:, :16]),
        dict(rotary_cos=cos[0], rotary_sin=cos[0]), dict(rotary_cos=torch.zeros(256, 33, dtype=bf), rotary_sin=torch.zeros(256, 33, dtype=bf)),
        dict(rotary_cos=cos[:0], rotary_sin=cos[:0]), dict(rotary_cos=cos[:, :0], rotary_sin=cos[:, :0]),
        dict(rotary_cos=torch.zeros(256, 64, dtype=bf)[:, ::2], rotary_sin=cos),  # non-unit last stride
        dict(rotary_cos=cos.to("meta"), rotary_sin=cos.to("meta")),
        dict(k_descale=torch.ones(2, 2)),                                         # descale with a 16-bit cache
        dict(K=K.to(torch.float8_e4m3fn), V=K.to(torch.float8_e4m3fn), k_descale=torch.ones(3, 2)),
        dict(K=K.float(), V=K.float(), Q=Q.float()),                              # k_new not in the cache's dtype
    ]
    for kw in bad:
        a = dict(base, **kw)
        with pytest.raises(ValueError):
            fa.flash_attention_kvcache_forward(a["Q"], a["K"], a["V"], a["lens"], "cpu", k_new=a["k_new"], v_new=a["v_new"],
                                               rotary_cos=a["rotary_cos"], rotary_sin=a["rotary_sin"], k_descale=a.get("k_descale"))
        if a["k_new"] is not None and a["v_new"] is not None and "Q" not in kw:
            with pytest.raises(ValueError):
                fa.kvcache_append(a["K"], a["V"], a["k_new"], a["v_new"], a["lens"], rotary_cos=a["rotary_cos"],
                                  rotary_sin=a["rotary_sin"], k_descale=a.get("k_descale"))
    with pytest.raises(ValueError):
        fa.kvcache_append(K, K, None, None, lens)
    with pytest.raises(ValueError):  # a table of the wrong B
        fa.kvcache_append(pool, pool, kn, kn, lens, block_table=torch.zeros(3, 4, dtype=torch.int32))
    # what is fine reaches the launch, which refuses CPU tensors
    k8 = K.to(torch.float8_e5m2)
    nhd = torch.zeros(2, 3, 2, 64, dtype=bf).transpose(1, 2)  # a flash-attn (B, N_new, H_kv, d) tensor
    for kw in (dict(), dict(rotary_cos=None, rotary_sin=None), dict(K=k8, V=k8, k_descale=torch.ones(2, 2)), dict(k_new=nhd, v_new=nhd),
               dict(K=pool, V=pool, table=table), dict(rotary_cos=cos[:, :8], rotary_sin=cos[:, :8])):
        a = dict(base, **kw)
        with pytest.raises(NotImplementedError):
            fa.flash_attention_kvcache_forward(a["Q"], a["K"], a["V"], a["lens"], "cpu", num_splits=1, k_new=a["k_new"], v_new=a["v_new"],
                                               rotary_cos=a["rotary_cos"], rotary_sin=a["rotary_sin"], k_descale=a.get("k_descale"),
                                               block_table=a.get("table"))
        with pytest.raises(NotImplementedError):
            fa.kvcache_append(a["K"], a["V"], a["k_new"], a["v_new"], a["lens"], rotary_cos=a["rotary_cos"], rotary_sin=a["rotary_sin"],
                              k_descale=a.get("k_descale"), block_table=a.get("table"))


def _tables(S, half, seed, dtype=torch.float32):
    ang = torch.rand(S, half, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 6.283
    return ang.cos().to(dtype), ang.sin().to(dtype)


@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("rd", [64, 32, 2])
def test_apply_rotary_against_fp64_complex_multiplication(interleaved, rd):
    """(x1 + i x2)(c + i s) in fp64 on the fp32 inputs.  Three roundings of relative size 2^-24 each give, to first order,
    |err| <= 2^-23 (|x1 c| + |x2 s|); the bar is 2^-22 (|x1| + |x2|)."""
    g = torch.Generator().manual_seed(rd + interleaved)
    x = torch.randn(3, 5, 7, 64, generator=g)
    cos, sin = _tables(40, rd // 2, 3)
    pos = torch.randint(0, 40, (3, 1, 7), generator=g)
    out = fa.apply_rotary(x, cos, sin, pos, interleaved)
    assert out.dtype == x.dtype and out.shape == x.shape
    xr = x[..., :rd].double()
    x1, x2 = (xr[..., 0::2], xr[..., 1::2]) if interleaved else (xr[..., :rd // 2], xr[..., rd // 2:])
    z = torch.complex(x1, x2) * torch.complex(cos.double(), sin.double())[torch.broadcast_to(pos, x.shape[:-1])]
    o = out[..., :rd].double()
    o1, o2 = (o[..., 0::2], o[..., 1::2]) if interleaved else (o[..., :rd // 2], o[..., rd // 2:])
    bar = 2.0 ** -22 * (x1.abs() + x2.abs())
    print(f"max err / bar: {((o1 - z.real).abs() / bar).max():.3f}, {((o2 - z.imag).abs() / bar).max():.3f}")
    assert ((o1 - z.real).abs() <= bar).all() and ((o2 - z.imag).abs() <= bar).all()
    assert torch.equal(bits(out[..., rd:]), bits(x[..., rd:]))  # columns >= rotary_dim: unchanged, bit for bit


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16, torch.float64])
def test_apply_rotary_interleaved_is_the_permuted_half_split_form(dtype):
    g = torch.Generator().manual_seed(5)
    rd, d = 24, 40
    x = torch.randn(2, 3, 4, d, generator=g).to(dtype)
    cos, sin = _tables(16, rd // 2, 9, dtype)
    pos = torch.randint(0, 16, (2, 3, 4), generator=g)
    # column 2i of the interleaved form is column i of the half-split form, 2i + 1 is i + rd / 2
    perm = torch.cat([torch.arange(0, rd, 2), torch.arange(1, rd, 2), torch.arange(rd, d)])
    a = fa.apply_rotary(x, cos, sin, pos, True)
    b = fa.apply_rotary(x[..., perm], cos, sin, pos, False)
    assert a.dtype == dtype and torch.equal(bits(a[..., perm]), bits(b))
    assert torch.equal(bits(a[..., rd:]), bits(x[..., rd:]))
    # positions are clamped into the tables
    assert torch.equal(bits(fa.apply_rotary(x, cos, sin, pos + 100, True)), bits(fa.apply_rotary(x, cos, sin, torch.tensor(15), True)))


def test_seqlens_out_restatement():
    cap = 256
    lens = torch.tensor([-3, 0, 1, cap - 1, cap, cap + 5], dtype=torch.int32)
    for n_new, want_start, want in ((1, [0, 0, 1, 255, 256, 256], [1, 1, 2, 256, 256, 256]),
                                    (3, [0, 0, 1, 255, 256, 256], [3, 3, 4, 256, 256, 256])):
        start, out = new_lengths(lens, n_new, cap)
        assert start.dtype == torch.int32 and out.dtype == torch.int32
        assert start.tolist() == want_start and out.tolist() == want
        # the same in numpy-style integer arithmetic, one sequence at a time
        assert out.tolist() == [min(min(max(int(n), 0), cap) + n_new, cap) for n in lens]
    # ... and the cache restatement drops what does not fit and touches nothing else
    K0 = torch.arange(6 * 1 * cap * 2, dtype=torch.float32).view(6, 1, cap, 2)
    kn = -torch.ones(6, 1, 3, 2)
    K, V, start, out = expected_append(K0, K0, kn, kn, lens)
    changed = (K != K0).any(-1)[:, 0]
    assert [row.nonzero().view(-1).tolist() for row in changed] == [[0, 1, 2], [0, 1, 2], [1, 2, 3], [255], [], []]
    assert torch.equal(K, V)
