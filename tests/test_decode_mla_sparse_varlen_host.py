"""Sparse MLA decode of packed queries (fa2_fwd_kvcache_mla_sparse_varlen, fa2_kvcache_mla_sparse_varlen_num_splits), the part that
needs no GPU: the two exported symbols, every argument error before any launch (fake pointers), the split heuristic against its
formula and against the fixed call's at B * N_q = total_q, which kernel a valid call launches first (a child process that sees no
device), and the Python wrapper's errors on CPU tensors.

    python tests/test_decode_mla_sparse_varlen_host.py --forms     the child: one JSON line, {"skipped": ...} or {name: [code, message]}"""
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

NEW = ("fa2_fwd_kvcache_mla_sparse_varlen", "fa2_kvcache_mla_sparse_varlen_num_splits")
MLA16 = 3
BF16, F16, F32 = _lib.FA2_DTYPE_BF16, _lib.FA2_DTYPE_F16, _lib.FA2_DTYPE_F32
E4M3 = _lib.FA2_DTYPE_F8E4M3
NONE = object()


def test_symbols_declared_bound_listed_and_exported():
    header = open(os.path.join(ROOT, "include", "fa2_fwd.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exports = open(os.path.join(ROOT, "flash_attention_dlrs_amd", "csrc", "fa2_exports.map")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS
        assert re.search(rf"\b{name}\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)), name
        assert re.search(rf"\bT {name}\b", out), name
        assert re.search(rf"\b{name};", exports), name
        assert getattr(_lib.lib(), name).argtypes is not None
    for name in ("flash_attention_mla_sparse_varlen_decode_forward", "check_mla_sparse_varlen_args"):
        assert name in fa.__all__ and callable(getattr(fa, name))
    assert callable(_lib.fa2_fwd_kvcache_mla_sparse_varlen) and callable(_lib.kvcache_mla_sparse_varlen_num_splits)


def _call(ptr=0x1000, v=None, cu=0x6000, indices=0x3000, index_strides=NONE, topk=200, table=None, kd=None, vd=None, B=3, H=16, H_kv=1,
          total_q=7, max_q=4, S_k=512, num_blocks=32, page_size=64, max_blocks=8, d=576, d_v=512, dtype=BF16, kv_dtype=None, num_splits=1,
          ws=None, ws_bytes=0, variant=0, kv_strides=None, v_strides=None, q_strides=NONE, scale=1.0):
    """contiguous unless `table`; the cache in `dtype` unless `kv_dtype`; V the first d_v columns of the rows unless `v`"""
    i64 = lambda t: None if t is None else (ctypes.c_int64 * len(t))(*t)
    rows = page_size if table else S_k
    ks = kv_strides or (H_kv * rows * d, rows * d, d, 1)
    if index_strides is NONE:
        index_strides = (H_kv * max(topk, 1), max(topk, 1), 1)
    if q_strides is NONE:
        q_strides = (H * d, d, 1)
    rc = _lib.lib().fa2_fwd_kvcache_mla_sparse_varlen(
        ptr, ptr, ptr if v is None else v, ptr, ptr, i64(q_strides), i64(ks), i64(v_strides or ks), i64((H * d_v, d_v, 1)), total_q, cu,
        None, indices, i64(index_strides), topk, table, max_blocks if table else 0, kd, vd, i64((1, 1)), i64((1, 1)), B, H, H_kv, total_q,
        max_q, num_blocks, rows, max_blocks, d, d_v, dtype, dtype if kv_dtype is None else kv_dtype, scale, num_splits, ws, ws_bytes,
        variant, None)
    return rc, _lib.lib().fa2_last_error().decode()


@pytest.mark.parametrize("kwargs,code,needle", [
    # what only the packed queries bring
    (dict(cu=None), -1, "kvcache varlen: null cu_seqlens_q"),
    (dict(total_q=0), -1, "kvcache varlen: total_q must be >= 1 (got 0)"), (dict(total_q=-5), -1, "total_q must be >= 1"),
    (dict(max_q=0), -1, "kvcache varlen: max_seqlen_q must be in [1, 2^28] (got 0)"), (dict(max_q=-1), -1, "max_seqlen_q must be in"),
    (dict(max_q=(1 << 28) + 1), -1, "max_seqlen_q must be in"), (dict(q_strides=None), -1, "kvcache varlen: null q_strides"),
    # what only the lists bring
    (dict(topk=0), -1, "topk must be in [1, 2^28] (got 0)"), (dict(topk=-3), -1, "topk must be in [1, 2^28]"),
    (dict(topk=(1 << 28) + 1), -1, "topk must be in [1, 2^28]"),
    (dict(indices=None), -1, "kvcache mla sparse: null indices"), (dict(index_strides=None), -1, "kvcache mla sparse: null index_strides"),
    (dict(index_strides=(200, 200, -1)), -1, "negative strides are not supported (index_strides)"),
    (dict(index_strides=(-200, 0, 1)), -1, "negative strides are not supported (index_strides)"),
    (dict(index_strides=(200, -200, 1)), -1, "negative strides are not supported (index_strides)"),
    # an fp8 cache brings its descales; descales go with an fp8 cache
    (dict(kv_dtype=E4M3), -1, "null k_descale with an fp8 cache"), (dict(kv_dtype=E4M3, kd=0x5000), -1, "null v_descale with an fp8 cache"),
    (dict(kd=0x5000), -1, "go with an fp8"), (dict(kv_dtype=99, kd=0x5000, vd=0x5000), -2, "kv_dtype_enum"),
    (dict(kv_dtype=E4M3, kd=0x5000, vd=0x5000, dtype=F32), -2, "must be FA2_DTYPE_F16 or FA2_DTYPE_BF16"),
    # the shape
    (dict(d=577), -2, "kvcache mla: d=577 must be in [1, 576]"), (dict(d_v=513), -2, "kvcache mla: d_v=513 must be in [1, 512]"),
    # the variants
    (dict(variant=2), -2, "kvcache mla sparse: unknown variant 2 (auto 0, generic 1, mla16 3)"),
    (dict(variant=-1), -2, "kvcache mla sparse: unknown variant -1"),
    # a forced matrix form on what it cannot run
    (dict(variant=MLA16, d=128, d_v=128), -2, "d = 576"), (dict(variant=MLA16, d=192, d_v=128), -2, "d = 576"),
    (dict(variant=MLA16, v=0x9000), -2, "aliasing"), (dict(variant=MLA16, dtype=F32), -2, "f16/bf16"),
    (dict(variant=MLA16, kv_strides=(512 * 1152, 512 * 1152, 1152, 2)), -2, "unit d-stride"),
    (dict(variant=MLA16, q_strides=(16 * 580, 580, 1)), -2, "16-byte"),
    # the workspace: 4 n total_q H (d_v + 1)
    (dict(num_splits=4), -1, "workspace"),
    (dict(num_splits=4, ws=0x2000, ws_bytes=4 * 4 * 7 * 16 * 513 - 1), -1, f"workspace of {4 * 4 * 7 * 16 * 513} bytes"),
    # a grid that does not fit: total_q * num_splits * head tiles
    (dict(total_q=1 << 28, num_splits=16, ws=0x2000, ws_bytes=1 << 62, variant=MLA16), -1,
     "kvcache mla sparse varlen: grid too large (total_q * num_splits * head tiles"),
    (dict(total_q=1 << 28, num_splits=16, ws=0x2000, ws_bytes=1 << 62, variant=1), -1,
     "kvcache mla sparse varlen: grid too large (total_q * num_splits * ceil(g / 16)"),
    # inherited
    (dict(B=0), -1, "B must"), (dict(B=65536), -1, "B must"), (dict(H=16, H_kv=3), -1, "H_kv"), (dict(S_k=0), -1, "S_k"),
    (dict(num_splits=129), -1, "num_splits"), (dict(num_splits=-1), -1, "num_splits"), (dict(ptr=None), -1, "null Q"),
    (dict(table=0x4000, page_size=0), -1, "page_size"), (dict(scale=float("nan")), -1, "scale is NaN"),
])
def test_argument_errors_before_any_launch(kwargs, code, needle):
    rc, msg = _call(**kwargs)
    assert rc == code, (rc, msg)
    assert needle in msg, msg


def _split_count(base, slots, waves, min_tiles):
    """fa2_decode_api.hip split_count"""
    if base >= 256:
        return 1
    return max(1, min(-(-waves * 256 // base), -(-slots // 64) // min_tiles, 128))


def test_split_heuristic_formula_and_the_fixed_call_at_equal_token_counts():
    n, fixed = _lib.kvcache_mla_sparse_varlen_num_splits, _lib.kvcache_mla_sparse_num_splits
    sizes = (1, 63, 64, 65, 200, 256, 511, 512, 2048, 4096, 65536, 1 << 28)
    for H, H_kv in ((16, 1), (128, 1), (40, 1), (64, 1), (65, 1), (1, 1), (32, 2), (256, 2)):
        g = H // H_kv
        for B, N_q in ((1, 1), (1, 2), (16, 1), (16, 2), (128, 1), (128, 2), (1, 1024), (3, 3), (65535, 1)):
            total_q = B * N_q
            prev = 0
            for topk in sizes:
                k = n(total_q, H, H_kv, topk, 576, 512, BF16)
                # one chip wave, four tiles per split, cap 128, on total_q * H_kv * head tiles workgroups
                assert k == _split_count(total_q * H_kv * -(-g // 64), topk, 1, 4), (total_q, H, H_kv, topk, k)
                assert 1 <= k <= 128 and k >= prev
                prev = k
                assert k == fixed(B, H, H_kv, N_q, topk, 576, 512, BF16) == n(total_q, H, H_kv, topk, 576, 512, F16)
                valu = _split_count(total_q * H_kv * -(-g // 16), topk, 2, 4)
                assert n(total_q, H, H_kv, topk, 576, 512, F32) == valu == n(total_q, H, H_kv, topk, 192, 128, BF16)
                assert valu == fixed(B, H, H_kv, N_q, topk, 576, 512, F32)
    assert n(0, 16, 1, 2048, 576, 512, BF16) == 1 and n(2, 16, 1, 0, 576, 512, BF16) == 1
    assert n(2, 16, 3, 2048, 576, 512, BF16) == 1  # no whole group: the call refuses it


def _forms():
    """the child: which kernel the first launch of a valid call is, read off the launch failure of a process without a device"""
    if torch.cuda.device_count() != 0:
        return {"skipped": "a device is visible"}
    out = {}
    fp8 = dict(kv_dtype=E4M3, kd=0x5000, vd=0x5000)
    for name, kw in (("auto", dict()), ("auto_fp8", fp8), ("auto_page64", dict(table=0x4000)), ("auto_page48", dict(table=0x4000, page_size=48)),
                     ("auto_page1", dict(table=0x4000, page_size=1, max_blocks=512)),
                     ("auto_split", dict(num_splits=2, ws=0x2000, ws_bytes=1 << 30)), ("forced", dict(variant=MLA16)),
                     ("forced_page48_fp8", dict(table=0x4000, page_size=48, variant=MLA16, **fp8)),
                     ("auto_stride0", dict(index_strides=(0, 0, 1))), ("generic", dict(variant=1)),
                     ("auto_own_v", dict(v=0x9000)), ("auto_dstride2", dict(kv_strides=(512 * 1152, 512 * 1152, 1152, 2))),
                     ("auto_d192", dict(d=192, d_v=128)), ("auto_f32", dict(dtype=F32)), ("forced_own_v", dict(v=0x9000, variant=MLA16))):
        out[name] = list(_call(**kw))
    return out


def test_form_selection():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    run = subprocess.run([sys.executable, os.path.abspath(__file__), "--forms"], env=env, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    got = json.loads(run.stdout.strip().splitlines()[-1])
    if "skipped" in got:
        pytest.skip(got["skipped"])
    for name in ("auto", "auto_fp8", "auto_page64", "auto_page48", "auto_page1", "auto_split", "forced", "forced_page48_fp8", "auto_stride0"):
        assert got[name][0] == -4 and "kvcache mla16 kernel launch failed" in got[name][1], (name, got[name])
    for name in ("generic", "auto_own_v", "auto_dstride2", "auto_d192", "auto_f32"):
        assert got[name][0] == -4 and "kvcache mla sparse generic kernel launch failed" in got[name][1], (name, got[name])
    assert got["forced_own_v"][0] == -2 and "aliasing" in got["forced_own_v"][1], got["forced_own_v"]


def test_python_wrapper_errors():
    bf = torch.bfloat16
    Q = torch.zeros(7, 16, 576, dtype=bf)
    KV = torch.zeros(3, 1, 128, 576, dtype=bf)
    idx = torch.zeros(7, 1, 40, dtype=torch.int32)
    cu = torch.tensor([0, 4, 4, 7], dtype=torch.int32)
    lens = torch.tensor([3, 100, 128], dtype=torch.int32)
    one = torch.ones(3, 1)
    pool, table = torch.zeros(9, 1, 48, 576, dtype=bf), torch.zeros(3, 4, dtype=torch.int32)

    def call(**kw):
        return fa.flash_attention_mla_sparse_varlen_decode_forward(kw.pop("Q", Q), kw.pop("KV", KV), kw.pop("idx", idx), kw.pop("cu", cu),
                                                                   kw.pop("max_q", 4), kw.pop("lens", lens), "cpu", **kw)

    for kw, needle in (
            (dict(causal=True), "no causal argument: the index list is the mask"), (dict(causal=False), "no causal argument"),
            (dict(window=(64, 0)), "no window argument: the index list is the mask"), (dict(window=None), "no window argument"),
            (dict(idx=idx.long()), "int32"), (dict(idx=idx[0, 0]), "indices"), (dict(idx=idx[None]), "indices"), (dict(idx=[1, 2]), "indices"),
            (dict(idx=idx[:6]), "indices must be"), (dict(idx=idx[..., :0]), "topk >= 1"),
            (dict(idx=torch.zeros(7, 2, 40, dtype=torch.int32)), "indices must be"),
            (dict(Q=Q[0]), "Q must"), (dict(Q=Q[:, None]), "Q must"), (dict(KV=KV[0]), "KV_cache"),
            (dict(cu=cu.long()), "cu_seqlens_q"), (dict(cu=cu[:1]), "cu_seqlens_q"), (dict(cu=cu[None]), "cu_seqlens_q"), (dict(cu=[0, 7]), "cu_seqlens_q"),
            (dict(max_q=0), "max_seqlen_q"), (dict(max_q=4.0), "max_seqlen_q"), (dict(max_q=True), "max_seqlen_q"),
            (dict(d_v=0), "d_v"), (dict(d_v=576), "d_v"), (dict(d_v=512.0), "d_v"), (dict(d_v=True), "d_v"),
            (dict(kv_descale=one), "kv_descale goes with an fp8"),
            (dict(KV=KV.to(torch.float8_e4m3fn)), "needs its kv_descale"), (dict(KV=KV.to(torch.float8_e5m2)), "needs its kv_descale"),
            (dict(KV=KV.to(torch.float8_e4m3fn), kv_descale=torch.ones(4, 1)), "kv_descale"),
            (dict(KV=KV.to(torch.float8_e4m3fn), kv_descale=one, Q=Q.float()), "fp8"),
            (dict(variant="mfma16"), "variant"), (dict(variant="mla17"), "variant"),
            (dict(Q=Q[..., :512]), "kvcache"), (dict(Q=Q.float()), "dtype"), (dict(lens=lens.long()), "cache_seqlens"), (dict(lens=lens[:2]), "cache_seqlens"),
            (dict(num_splits=129), "num_splits"), (dict(num_splits=-1), "num_splits"), (dict(num_splits=2.0), "num_splits"),
            (dict(KV=torch.zeros(3, 3, 128, 576, dtype=bf)), "H"),
            (dict(KV=pool, block_table=table[:2]), "block_table"), (dict(KV=pool, block_table=table.long()), "block_table")):
        with pytest.raises(ValueError, match=needle):
            call(**kw)
    with pytest.raises(TypeError, match="unexpected keyword"):
        call(kv_new=KV)  # the append side is mla_kvcache_append_varlen, called first
    # what is fine reaches the launch, which refuses CPU tensors
    for kw in (dict(), dict(variant="mla16"), dict(variant="generic", num_splits=3), dict(lens=None), dict(idx=idx[:, 0]),
               dict(idx=idx[:, :, ::2]), dict(idx=idx[:1].expand(7, -1, -1)), dict(KV=pool, block_table=table),
               dict(KV=KV.to(torch.float8_e5m2), kv_descale=one), dict(KV=KV[..., :192], Q=Q[..., :192], d_v=128),
               dict(KV=KV.float(), Q=Q.float()), dict(KV=torch.zeros(3, 2, 128, 576, dtype=bf), idx=idx[:, 0]),
               dict(KV=torch.zeros(3, 2, 128, 576, dtype=bf), idx=idx.expand(-1, 2, -1)), dict(max_q=1 << 28)):
        with pytest.raises(NotImplementedError):
            call(**kw)
    # the pure check alone takes the same arguments
    fa.check_mla_sparse_varlen_args(Q, KV, idx, cu, 4, lens)
    fa.check_mla_sparse_varlen_args(Q, KV, idx[:, 0], cu, 4, None, 512, 3)
    with pytest.raises(ValueError, match="d_v"):
        fa.check_mla_sparse_varlen_args(Q, KV, idx, cu, 4, lens, 576)


if __name__ == "__main__":
    if sys.argv[1:] != ["--forms"]:
        sys.exit(__doc__)
    print(json.dumps(_forms()))
