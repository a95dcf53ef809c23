"""Packed queries over the latent cache (fa2_fwd_kvcache_mla_varlen, fa2_kvcache_mla_varlen_num_splits, fa2_fwd_kvcache_mla_varlen_append),
the part that needs no GPU: the three exported symbols, every argument error before any launch (fake pointers), the split heuristic
against its formula, which kernel a valid call launches first (a child process that sees no device), and the Python wrapper's errors
on CPU tensors.

    python tests/test_decode_mla_varlen_host.py --forms     the child: one JSON line, {"skipped": ...} or {name: [code, message]}"""
import ctypes
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import pytest
import torch

import flash_attention_dlrs_amd as fa
from flash_attention_dlrs_amd import _lib

NEW = ("fa2_fwd_kvcache_mla_varlen", "fa2_kvcache_mla_varlen_num_splits", "fa2_fwd_kvcache_mla_varlen_append")
MLA16 = 3
BF16, F32 = _lib.FA2_DTYPE_BF16, _lib.FA2_DTYPE_F32


def test_symbols_declared_bound_and_listed():
    header = open(os.path.join(ROOT, "include", "fa2_fwd.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exports = open(os.path.join(ROOT, "flash_attention_dlrs_amd", "csrc", "fa2_exports.map")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS
        assert re.search(rf"\b{name}\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)), name
        assert re.search(rf"\bT {name}\b", out), name
        assert re.search(rf"\b{name};", exports), name
    assert _lib.KVCACHE_MLA_VARIANTS == {"auto": 0, "generic": 1, "mla16": MLA16}
    for name in ("flash_attention_mla_varlen_decode_forward", "check_mla_varlen_args"):
        assert name in fa.__all__ and callable(getattr(fa, name))


def _call(ptr=0x1000, cu=0x3000, table=None, table_stride=None, descale=None, B=3, H=16, H_kv=1, total_q=7, max_q=4, S_k=512, num_blocks=32,
          page_size=64, max_blocks=8, d=576, d_v=512, dtype=BF16, kv_dtype=None, window=(-1, -1), num_splits=1, ws=None, ws_bytes=0,
          variant=0, kv_strides=None, q_strides=None, scale=1.0):
    """contiguous unless `table`; the cache in `dtype` unless `kv_dtype`"""
    i64 = lambda v: (ctypes.c_int64 * len(v))(*v)
    rows = page_size if table else S_k
    rc = _lib.lib().fa2_fwd_kvcache_mla_varlen(
        ptr, ptr, ptr, ptr, i64(q_strides or (H * d, d, 1)), i64(kv_strides or (H_kv * rows * d, rows * d, d, 1)), i64((H * d_v, d_v, 1)),
        total_q, cu, None, table, (max_blocks if table_stride is None else table_stride) if table else 0, descale, i64((1, 1)),
        B, H, H_kv, total_q, max_q, S_k, num_blocks, page_size, max_blocks, d, d_v, dtype, dtype if kv_dtype is None else kv_dtype, 0, scale,
        window[0], window[1], num_splits, ws, ws_bytes, variant, None)
    return rc, _lib.lib().fa2_last_error().decode()


@pytest.mark.parametrize("kwargs,code,needle", [
    (dict(cu=None), -1, "null cu_seqlens_q"),
    (dict(total_q=0), -1, "total_q must be >= 1"), (dict(total_q=-5), -1, "total_q must be >= 1"),
    (dict(max_q=0), -1, "max_seqlen_q must be in [1, 2^28]"), (dict(max_q=(1 << 28) + 1), -1, "max_seqlen_q must be in [1, 2^28]"),
    (dict(total_q=1 << 30, H=65535), -1, "total_q * H must be <= 2^40"),
    (dict(d=577), -2, "kvcache mla: d=577 must be in [1, 576]"),
    (dict(d_v=0), -2, "kvcache mla: d_v=0 must be in [1, 512]"), (dict(d_v=513), -2, "kvcache mla: d_v=513 must be in [1, 512]"),
    # the d 64 / 128 matrix form is no variant of this call, nor is an unknown one: the latent call's text
    (dict(variant=2), -2, "kvcache mla: unknown variant 2 (auto 0, generic 1, mla16 3)"),
    (dict(variant=7), -2, "kvcache mla: unknown variant 7"), (dict(variant=-1), -2, "kvcache mla: unknown variant -1"),
    (dict(descale=0x5000), -1, "go with an fp8 cache"),
    # the workspace: 4 n total_q H (d_v + 1), d's 576 columns are never asked for
    (dict(num_splits=4), -1, "workspace"),
    (dict(num_splits=4, ws=0x2000, ws_bytes=4 * 4 * 7 * 16 * 513 - 1), -1, f"workspace of {4 * 4 * 7 * 16 * 513} bytes"),
    (dict(num_splits=3, total_q=70, H=128, ws=0x2000, ws_bytes=4 * 3 * 70 * 128 * 513 - 1), -1, f"workspace of {4 * 3 * 70 * 128 * 513} bytes"),
    # a forced matrix form on what it cannot run
    (dict(variant=MLA16, table=0x4000, page_size=48), -2, "page_size % 64"),
    (dict(variant=MLA16, kv_strides=(512 * 1152, 512 * 1152, 1152, 2)), -2, "unit d-stride"),
    (dict(variant=MLA16, q_strides=(16 * 580, 580, 1)), -2, "16-byte"),
    (dict(variant=MLA16, d=192, d_v=128), -2, "d = 576"), (dict(variant=MLA16, dtype=F32), -2, "f16/bf16"),
    # inherited
    (dict(B=0), -1, "B must"), (dict(H=16, H_kv=3), -1, "H_kv"), (dict(S_k=0), -1, "S_k"), (dict(window=(-2, 0)), -1, "window"),
    (dict(num_splits=129), -1, "num_splits"), (dict(kv_dtype=99, descale=0x5000), -2, "kv_dtype_enum"),
    (dict(table=0x4000, page_size=0), -1, "page_size"),
])
def test_argument_errors_before_any_launch(kwargs, code, needle):
    rc, msg = _call(**kwargs)
    assert rc == code, (rc, msg)
    assert needle in msg, msg


def test_workspace_helper_is_the_packed_one_on_d_v():
    for total_q, H, n in ((7, 16, 4), (70, 128, 3), (1, 1, 2)):
        assert _lib.kvcache_varlen_workspace_bytes(total_q, H, 512, n) == 4 * n * total_q * H * 513


def _split_count(base, S_k):
    """fa2_decode_api.hip split_count at the packed latent call's constants: one wave of 256 workgroups, splits of at least eight key
    tiles (the split sweep of benchmarks/bench_mla_varlen.py moved the fixed call's four: DESIGN.md, "MLA decode: packed queries")"""
    if base >= 256:
        return 1
    return max(1, min(-(-256 // base), -(-S_k // 64) // 8, 128))


def _formula(B, H, H_kv, total_q, max_q, S_k):
    g = H // H_kv
    return _split_count(H_kv * min(B * -(-g * max_q // 64), -(-g * total_q // 64) + B), S_k)


def test_split_heuristic_is_the_formula():
    n = _lib.kvcache_mla_varlen_num_splits
    sizes = (1, 63, 64, 65, 300, 2048, 4096, 8192, 65536, 1 << 20, 1 << 28)
    for H, H_kv in ((16, 1), (128, 1), (40, 1), (5, 1), (1, 1), (32, 2), (64, 1)):
        for B, total_q, max_q in ((1, 1, 1), (1, 256, 256), (9, 163, 70), (64, 128, 2), (16, 64, 4), (64, 319, 256), (64, 64, 1),
                                  (300, 300, 1), (65535, 65535, 1), (2, 1 << 20, 1 << 19)):
            prev = 0
            for S_k in sizes:
                k = n(B, H, H_kv, total_q, max_q, S_k, 576, 512, BF16)
                assert k == _formula(B, H, H_kv, total_q, max_q, S_k), (B, H, H_kv, total_q, max_q, S_k, k)
                assert 1 <= k <= 128 and k >= prev                     # in range, monotone in S_k
                prev = k
                assert k == n(B, H, H_kv, total_q, max_q, S_k, 576, 512, _lib.FA2_DTYPE_F16)
                # any other shape is the VALU form's packed count: per query head and 16 rows
                valu = _lib.kvcache_varlen_num_splits(B, H, H_kv, total_q, max_q, S_k, 40, F32)
                assert n(B, H, H_kv, total_q, max_q, S_k, 576, 512, F32) == valu
                assert n(B, H, H_kv, total_q, max_q, S_k, 192, 128, BF16) == valu
    # one token per sequence: min(B ceil(g / 64), ceil(g B / 64) + B) workgroups' worth, which is the fixed latent call's count at N_q = 1
    for H in (1, 5, 16, 40, 64, 65, 128):
        for B in (1, 2, 16, 64, 128, 300):
            g = H
            for S_k in sizes:
                k = n(B, H, 1, B, 1, S_k, 576, 512, BF16)
                assert k == _split_count(min(B * -(-g // 64), -(-g * B // 64) + B), S_k)
                assert min(B * -(-g // 64), -(-g * B // 64) + B) == B * -(-g // 64)
                assert k <= _lib.kvcache_mla_num_splits(B, H, 1, 1, S_k, 576, 512, BF16)     # (longer splits than the fixed call's)
    assert n(0, 16, 1, 4, 2, 8192, 576, 512, BF16) == 1 and n(2, 16, 1, 0, 2, 8192, 576, 512, BF16) == 1
    assert n(2, 16, 3, 4, 2, 8192, 576, 512, BF16) == _lib.kvcache_varlen_num_splits(2, 16, 3, 4, 2, 8192, 40, BF16)  # no whole group


def _forms():
    """the child: which kernel the first launch of a valid call is, read off the launch failure of a process without a device"""
    if torch.cuda.device_count() != 0:
        return {"skipped": "a device is visible"}
    out = {}
    for name, kw in (("auto", dict()), ("auto_fp8", dict(kv_dtype=_lib.FA2_DTYPE_F8E4M3, descale=0x5000)),
                     ("auto_paged", dict(table=0x4000, page_size=128)), ("auto_split", dict(num_splits=2, ws=0x2000, ws_bytes=1 << 30)),
                     ("forced", dict(variant=MLA16)), ("generic", dict(variant=1)),
                     ("auto_page48", dict(table=0x4000, page_size=48)), ("forced_page48", dict(table=0x4000, page_size=48, variant=MLA16)),
                     ("auto_dstride2", dict(kv_strides=(512 * 1152, 512 * 1152, 1152, 2))),
                     ("forced_dstride2", dict(kv_strides=(512 * 1152, 512 * 1152, 1152, 2), variant=MLA16)),
                     ("auto_d192", dict(d=192, d_v=128)), ("auto_f32", dict(dtype=F32))):
        out[name] = list(_call(**kw))
    return out


def test_form_selection():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    run = subprocess.run([sys.executable, os.path.abspath(__file__), "--forms"], env=env, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    got = json.loads(run.stdout.strip().splitlines()[-1])
    if "skipped" in got:
        pytest.skip(got["skipped"])
    for name in ("auto", "auto_fp8", "auto_paged", "auto_split", "forced"):
        assert got[name][0] == -4 and "kvcache mla16 kernel launch failed" in got[name][1], (name, got[name])
    for name in ("generic", "auto_page48", "auto_dstride2", "auto_d192", "auto_f32"):
        assert got[name][0] == -4 and "kvcache generic kernel launch failed" in got[name][1], (name, got[name])
    for name, needle in (("forced_page48", "page_size % 64"), ("forced_dstride2", "unit d-stride")):
        assert got[name][0] == -2 and "kvcache mla16 kernel" in got[name][1] and needle in got[name][1], (name, got[name])


def test_python_wrapper_errors():
    bf = torch.bfloat16
    Q = torch.zeros(7, 16, 576, dtype=bf)
    KV = torch.zeros(3, 1, 128, 576, dtype=bf)
    cu = torch.tensor([0, 2, 3, 7], dtype=torch.int32)
    lens = torch.tensor([3, 100, 128], dtype=torch.int32)
    one = torch.ones(3, 1)
    new = torch.zeros(7, 1, 576, dtype=bf)
    rot = torch.zeros(256, 32, dtype=bf)
    pool, table = torch.zeros(9, 1, 64, 576, dtype=bf), torch.zeros(3, 4, dtype=torch.int32)

    def call(**kw):
        return fa.flash_attention_mla_varlen_decode_forward(kw.pop("Q", Q), kw.pop("KV", KV), kw.pop("cu", cu), kw.pop("max_q", 4),
                                                            kw.pop("lens", lens), "cpu", **kw)

    for kw, needle in (
            (dict(Q=Q[None]), "packed"), (dict(Q=Q[0]), "packed"), (dict(Q=Q[:0]), "packed"), (dict(KV=KV[0]), "KV_cache"),
            (dict(cu=cu.long()), "cu_seqlens_q"), (dict(cu=cu[:1]), "cu_seqlens_q"), (dict(cu=cu[None]), "cu_seqlens_q"),
            (dict(cu=torch.zeros(8, dtype=torch.int32)[::2]), "cu_seqlens_q"), (dict(cu=cu[:3]), "K_cache"),
            (dict(max_q=0), "max_seqlen_q"), (dict(max_q=4.0), "max_seqlen_q"), (dict(max_q=True), "max_seqlen_q"),
            (dict(d_v=0), "d_v"), (dict(d_v=576), "d_v"), (dict(d_v=600), "d_v"), (dict(d_v=512.0), "d_v"), (dict(d_v=True), "d_v"),
            (dict(kv_descale=one), "kv_descale goes with an fp8"),
            (dict(rotary_cos=rot, rotary_sin=rot), "need kv_new"), (dict(rotary_sin=rot), "go together"),
            (dict(kv_new=new, rotary_cos=rot), "go together"),
            (dict(kv_new=new[:5]), "total_q"), (dict(kv_new=new.to(torch.float16)), "dtype"), (dict(kv_new=new[None]), "kv_new"),
            (dict(kv_new=(new[..., :512], new[..., 512:544])), "kv_new"), (dict(kv_new=new, lens=None), "cache_seqlens"),
            (dict(kv_new=new, rotary_cos=torch.zeros(256, 40, dtype=bf), rotary_sin=torch.zeros(256, 40, dtype=bf)), "rotary"),
            (dict(variant="mfma16"), "variant"), (dict(variant="mla17"), "variant"),
            (dict(Q=Q[..., :512]), "kvcache"), (dict(Q=Q.float()), "dtype"), (dict(lens=lens.long()), "cache_seqlens"),
            (dict(num_splits=129), "num_splits"), (dict(window=(-2, 0)), "window"),
            (dict(KV=torch.zeros(3, 3, 128, 576, dtype=bf)), "H"),
            (dict(KV=torch.zeros(3, 1, 128, 600, dtype=bf), Q=torch.zeros(7, 16, 600, dtype=bf)), "576"),
            (dict(KV=pool, block_table=table[:2]), "block_table"), (dict(KV=pool, block_table=table.long()), "block_table"),
            (dict(KV=KV.to(torch.float8_e4m3fn), Q=Q.float()), "fp8"),
            (dict(KV=KV.to(torch.float8_e4m3fn), kv_descale=torch.ones(4, 1)), "kv_descale")):
        with pytest.raises(ValueError, match=needle):
            call(**kw)
    # what is fine reaches the launch, which refuses CPU tensors
    for kw in (dict(), dict(variant="mla16"), dict(variant="generic", num_splits=3), dict(lens=None), dict(causal=True, window=(64, 0)),
               dict(KV=pool, block_table=table), dict(KV=KV.to(torch.float8_e5m2), kv_descale=one), dict(KV=KV.to(torch.float8_e4m3fn)),
               dict(KV=KV[..., :192], Q=Q[..., :192], d_v=128), dict(KV=KV.float(), Q=Q.float()), dict(Q=torch.zeros(7, 16, 600, dtype=bf)[..., :576]),
               dict(kv_new=new), dict(kv_new=(new[..., :512], new[..., 512:]), rotary_cos=rot, rotary_sin=rot, rotary_interleaved=True),
               dict(kv_new=new, KV=pool, block_table=table, causal=True), dict(cu=torch.tensor([0, 0, 9, 4], dtype=torch.int32))):
        with pytest.raises(NotImplementedError):
            call(**kw)
    # the pure check alone takes the same arguments
    fa.check_mla_varlen_args(Q, KV, cu, 4, lens)
    with pytest.raises(ValueError, match="d_v"):
        fa.check_mla_varlen_args(Q, KV, cu, 4, lens, 576)


if __name__ == "__main__":
    if sys.argv[1:] != ["--forms"]:
        sys.exit(__doc__)
    print(json.dumps(_forms()))
