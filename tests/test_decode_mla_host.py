"""MLA decode (fa2_fwd_kvcache_mla: a value head size of its own, a V that may alias K), the part that needs no GPU: the two
exported symbols, every argument error before any launch (fake pointers), the workspace formula on d_v, the split heuristic, and
the Python wrapper's errors on CPU tensors."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from conftest import ROOT

import flash_attention_dlrs_amd as fa
from flash_attention_dlrs_amd import _lib

NEW = ("fa2_fwd_kvcache_mla", "fa2_kvcache_mla_num_splits")
MLA16 = 3


def test_symbols_declared_bound_and_listed():
    header = open(os.path.join(ROOT, "include", "fa2_fwd.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exports = open(os.path.join(ROOT, "flash_attention_dlrs_amd", "csrc", "fa2_exports.map")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS
        assert re.search(rf"\b{name}\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)), name
        assert re.search(rf"\bT {name}\b", out), name
        assert re.search(rf"\b{name};", exports), name
    assert re.search(r"#define FA2_KVCACHE_VARIANT_MLA16 3\b", header)
    assert _lib.KVCACHE_MLA_VARIANTS == {"auto": 0, "generic": 1, "mla16": MLA16}
    assert callable(_lib.fa2_fwd_kvcache_mla) and callable(fa.flash_attention_mla_decode_forward)
    assert "flash_attention_mla_decode_forward" in fa.__all__


def _call(ptr=0x1000, v_ptr=None, null=None, table=None, table_stride=None, B=2, H=16, H_kv=1, N_q=1, num_blocks=32, page_size=512,
          max_blocks=8, d=576, d_v=512, dtype=_lib.FA2_DTYPE_BF16, window=(-1, -1), num_splits=1, ws=None, ws_bytes=0, variant=0,
          k_strides=None, v_strides=None, q_strides=None, scale=1.0):
    """contiguous by default (block_table null: page_size carries S_k); V aliases K unless v_ptr / v_strides say otherwise"""
    i64 = lambda v: (ctypes.c_int64 * len(v))(*v)
    qs = q_strides or (H * N_q * d, N_q * d, d, 1)
    os_ = (H * N_q * d_v, N_q * d_v, d_v, 1)
    ks = k_strides or (H_kv * page_size * d, page_size * d, d, 1)
    vs = v_strides or ks
    p = {n: ptr for n in "QKVOL"}
    if v_ptr is not None:
        p["V"] = v_ptr
    if null:
        p[null] = None
    rc = _lib.lib().fa2_fwd_kvcache_mla(p["Q"], p["K"], p["V"], p["O"], p["L"], i64(qs), i64(ks), i64(vs), i64(os_), i64((H * N_q, N_q)),
                                        None, table, (max_blocks if table_stride is None else table_stride) if table else 0, B, H, H_kv,
                                        N_q, num_blocks, page_size, max_blocks, d, d_v, dtype, 0, scale, window[0], window[1],
                                        num_splits, ws, ws_bytes, variant, None)
    return rc, _lib.lib().fa2_last_error().decode()


PAGED = dict(table=0x4000, page_size=64)


@pytest.mark.parametrize("kwargs,code,needle", [
    # the head sizes
    (dict(d=577), -2, "[1, 576]"), (dict(d=0), -2, "[1, 576]"), (dict(d_v=513), -2, "[1, 512]"), (dict(d_v=0), -2, "[1, 512]"),
    (dict(d=577, d_v=513), -2, "[1, 576]"),
    # a forced matrix form on what it cannot run: the message names the rule
    (dict(variant=MLA16, d=128, d_v=128), -2, "d = 576"), (dict(variant=MLA16, d=128, d_v=64), -2, "d = 576"),
    (dict(variant=MLA16, d_v=256), -2, "d_v = 512"),
    (dict(variant=MLA16, v_ptr=0x9000), -2, "aliasing"),                                       # a V of its own
    (dict(variant=MLA16, v_strides=(512 * 512, 512 * 512, 512, 1)), -2, "aliasing"),           # ... or its own strides
    (dict(variant=MLA16, dtype=_lib.FA2_DTYPE_F32), -2, "f16/bf16"),
    (dict(variant=MLA16, scale=0.0), -2, "scale > 0"),
    (dict(variant=MLA16, k_strides=(512 * 1152, 512 * 1152, 1152, 2)), -2, "unit d-stride"),
    (dict(variant=MLA16, k_strides=(512 * 580, 512 * 580, 580, 1)), -2, "16-byte"),
    (dict(variant=MLA16, ptr=0x1004), -2, "16-byte"),
    (dict(variant=MLA16, table=0x4000, page_size=16), -2, "page_size % 64"),
    (dict(variant=MLA16, table=0x4000, page_size=48), -2, "page_size % 64"),
    # the d 64 / 128 matrix form is no variant of this call, nor is an unknown one
    (dict(variant=2), -2, "variant"), (dict(variant=7), -2, "variant"), (dict(variant=-1), -2, "variant"),
    # the paged arguments
    (dict(PAGED, page_size=0), -1, "page_size"), (dict(PAGED, max_blocks=0), -1, "max_blocks"), (dict(PAGED, num_blocks=0), -1, "num_blocks"),
    (dict(PAGED, page_size=-64), -1, "page_size"), (dict(PAGED, max_blocks=(1 << 22) + 1), -1, "2^28"),
    (dict(PAGED, max_blocks=1 << 30, page_size=1 << 30), -1, "2^28"), (dict(PAGED, table_stride=-1), -1, "block_table_stride"),
    # contiguous: page_size carries S_k
    (dict(page_size=0), -1, "S_k"), (dict(page_size=(1 << 28) + 1), -1, "S_k"),
    # the workspace: d_v columns
    (dict(num_splits=4), -1, "workspace"), (dict(num_splits=4, ws=0x2000, ws_bytes=4 * 4 * 2 * 16 * 1 * 513 - 1), -1, "workspace"),
    (dict(num_splits=0, B=1, page_size=8192), -1, "workspace"),      # auto resolves to more than 1 here
    (dict(PAGED, num_splits=0, B=1, max_blocks=128), -1, "workspace"),
    # inherited from the other entry points
    (dict(null="Q"), -1, "null Q"), (dict(null="K"), -1, "null K"), (dict(null="V"), -1, "null V"), (dict(null="O"), -1, "null O"),
    (dict(null="L"), -1, "null L"),
    (dict(B=0), -1, "B must"), (dict(B=65536), -1, "B must"), (dict(H=0), -1, "H must"), (dict(H_kv=0), -1, "H_kv"),
    (dict(H=16, H_kv=3), -1, "H_kv"), (dict(N_q=0), -1, "N_q"), (dict(window=(-2, 0)), -1, "window"),
    (dict(num_splits=-1), -1, "num_splits"), (dict(num_splits=129), -1, "num_splits"),
    (dict(k_strides=(-1, 576, 576, 1)), -1, "negative"), (dict(q_strides=(576, 576, -576, 1)), -1, "negative"),
    (dict(scale=float("nan")), -1, "NaN"),
    (dict(dtype=_lib.FA2_DTYPE_F8E4M3), -2, "fp8"), (dict(dtype=_lib.FA2_DTYPE_F8E5M2), -2, "fp8"), (dict(dtype=99), -2, "dtype"),
])
def test_argument_errors_before_any_launch(kwargs, code, needle):
    rc, msg = _call(**kwargs)
    assert rc == code, (rc, msg)
    assert needle in msg, msg


def test_workspace_accepts_exactly_the_d_v_formula():
    """one byte less than fa2_kvcache_workspace_bytes(B, H, N_q, d_v, n) is refused above; d's 576 columns are never asked for"""
    for B, H, N_q, d_v, n in ((2, 16, 1, 512, 4), (1, 128, 2, 512, 16), (3, 8, 2, 128, 3)):
        need = _lib.kvcache_workspace_bytes(B, H, N_q, d_v, n)
        assert need == 4 * n * B * H * N_q * (d_v + 1)
        rc, msg = _call(B=B, H=H, N_q=N_q, d_v=d_v, d=576 if d_v == 512 else 192, num_splits=n, ws=0x2000, ws_bytes=need - 1)
        assert rc == -1 and "workspace" in msg and str(need) in msg, (rc, msg)
    assert _lib.kvcache_workspace_bytes(2, 16, 1, 576, 4) == 2 ** 63 - 1      # the existing helper's own limit stays [1, 512]


def test_existing_entry_points_keep_their_limits():
    i64 = lambda v: (ctypes.c_int64 * len(v))(*v)
    s = (8 * 576, 576, 576, 1)
    for d, variant, needle in ((576, 0, "[1, 512]"), (513, 0, "[1, 512]"), (64, MLA16, "variant")):
        rc = _lib.lib().fa2_fwd_kvcache_variant(0x1000, 0x1000, 0x1000, 0x1000, 0x1000, i64(s), i64(s), i64(s), i64(s), i64((8, 1)), None,
                                                1, 8, 1, 1, 64, d, _lib.FA2_DTYPE_BF16, 0, 1.0, -1, -1, 1, None, 0, None, variant)
        assert rc == -2 and needle in _lib.lib().fa2_last_error().decode()
    assert "mla16" not in _lib.KVCACHE_VARIANTS


def test_split_heuristic_range_and_monotone_in_s_k():
    bf, f32 = _lib.FA2_DTYPE_BF16, _lib.FA2_DTYPE_F32
    n = _lib.kvcache_mla_num_splits
    for H, N_q in ((16, 1), (128, 1), (128, 2), (40, 3)):
        for B in (1, 2, 16, 64, 128, 65535):
            prev = 0
            for S_k in (1, 63, 64, 65, 300, 2048, 4096, 8192, 65536, 1 << 20, 1 << 28):
                k = n(B, H, 1, N_q, S_k, 576, 512, bf)
                assert 1 <= k <= 128 and k <= -(-S_k // 64)
                assert k >= prev, (H, N_q, B, S_k, k, prev)
                prev = k
    # the matrix form counts B * H_kv * ceil(g N_q / 64) workgroups, one per CU
    assert n(256, 16, 1, 1, 65536, 576, 512, bf) == 1 and n(128, 128, 1, 1, 65536, 576, 512, bf) == 1
    assert n(1, 16, 1, 1, 65536, 576, 512, bf) == 128 and n(1, 128, 1, 1, 65536, 576, 512, bf) == 128
    assert n(16, 128, 1, 1, 65536, 576, 512, bf) == 8 == n(16, 64, 1, 2, 65536, 576, 512, bf) == n(32, 64, 1, 1, 65536, 576, 512, bf)
    assert n(1, 16, 1, 1, 8192, 576, 512, bf) == 32                              # at least four key tiles per split
    # any other shape is the VALU form's count: per query head and 16 rows
    assert n(1, 16, 1, 1, 8192, 576, 512, f32) == _lib.kvcache_num_splits(1, 16, 1, 1, 8192, 40, f32)
    assert n(1, 16, 1, 1, 8192, 192, 128, bf) == _lib.kvcache_num_splits(1, 16, 1, 1, 8192, 40, bf)
    assert n(0, 16, 1, 1, 8192, 576, 512, bf) == 1


def test_python_wrapper_errors():
    Q = torch.zeros(2, 16, 1, 576, dtype=torch.bfloat16)
    KV = torch.zeros(2, 1, 128, 576, dtype=torch.bfloat16)
    V = KV[..., :512]
    lens = torch.tensor([3, 100], dtype=torch.int32)
    one = torch.ones(2, 1)
    new = torch.zeros(2, 1, 1, 576, dtype=torch.bfloat16)
    rot = torch.zeros(256, 32, dtype=torch.bfloat16)
    call = lambda **kw: fa.flash_attention_kvcache_forward(kw.pop("Q", Q), kw.pop("K", KV), kw.pop("V", V), kw.pop("lens", lens), "cpu", **kw)
    # out of scope with d_v != d: the message names the argument
    for kw, needle in ((dict(k_descale=one), "k_descale"), (dict(v_descale=one), "v_descale"),
                       (dict(k_new=new, v_new=new[..., :512]), "k_new"), (dict(v_new=new[..., :512]), "v_new"),
                       (dict(rotary_cos=rot, rotary_sin=rot), "rotary_cos"), (dict(rotary_sin=rot), "rotary_sin"),
                       (dict(K=KV.to(torch.float8_e4m3fn), V=V.to(torch.float8_e4m3fn)), "fp8"),
                       (dict(K=KV.to(torch.float8_e5m2), V=V.to(torch.float8_e5m2), k_descale=one), "fp8"),
                       (dict(variant="mfma16"), "variant"), (dict(variant="mla17"), "variant")):
        with pytest.raises(ValueError, match=needle):
            call(**kw)
    # V differing from K on any axis but the last; other bad shapes and dtypes
    for kw in (dict(V=V[:1]), dict(V=torch.zeros(2, 2, 128, 512, dtype=torch.bfloat16)), dict(V=V[:, :, :64]), dict(V=V[0]),
               dict(V=V.float()), dict(Q=Q[..., :512]), dict(Q=Q[:1]), dict(lens=lens.long()), dict(num_splits=129),
               dict(window=(-2, 0)), dict(K=torch.zeros(2, 1, 128, 600, dtype=torch.bfloat16), Q=torch.zeros(2, 16, 1, 600, dtype=torch.bfloat16)),
               dict(K=torch.zeros(2, 3, 128, 576, dtype=torch.bfloat16), V=torch.zeros(2, 3, 128, 512, dtype=torch.bfloat16))):
        with pytest.raises(ValueError):
            call(**kw)
    # equal shapes stay on today's path: "mla16" is no variant there
    with pytest.raises(ValueError, match="variant"):
        call(V=KV, variant="mla16")
    # what is fine reaches the launch, which refuses CPU tensors
    pool, table = torch.zeros(9, 1, 64, 576, dtype=torch.bfloat16), torch.zeros(2, 4, dtype=torch.int32)
    for kw in (dict(), dict(variant="mla16"), dict(variant="generic", num_splits=3), dict(lens=None),
               dict(V=torch.zeros(2, 1, 128, 512, dtype=torch.bfloat16)), dict(K=KV[..., :192], V=KV[..., :128], Q=Q[..., :192]),
               dict(K=pool, V=pool[..., :512], block_table=table), dict(K=KV.float(), V=V.float(), Q=Q.float())):
        with pytest.raises(NotImplementedError):
            call(**kw)
    # the convenience form
    with pytest.raises(NotImplementedError):
        fa.flash_attention_mla_decode_forward(Q, KV, lens, "cpu")
    with pytest.raises(NotImplementedError):
        fa.flash_attention_mla_decode_forward(Q, pool, lens, "cpu", block_table=table, variant="mla16", causal=True)
    for kw in (dict(d_v=576), dict(d_v=0), dict(d_v=512.0), dict(d_v=True)):
        with pytest.raises(ValueError, match="d_v"):
            fa.flash_attention_mla_decode_forward(Q, KV, lens, "cpu", **kw)
    with pytest.raises(ValueError):
        fa.flash_attention_mla_decode_forward(Q, KV[0], lens, "cpu")
