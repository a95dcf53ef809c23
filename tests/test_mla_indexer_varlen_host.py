"""The MLA indexer over packed queries (fa2_mla_indexer_logits_varlen, fa2_topk_indices_varlen, fa2_mla_indexer_topk_varlen,
fa2_mla_indexer_varlen_workspace_bytes), the part that needs no GPU: the four exported symbols, every argument error before any launch
(fake pointers), which kernel a valid call launches first (a child process that sees no device), and the Python surface's errors on
CPU tensors.

    python tests/test_mla_indexer_varlen_host.py --forms     the child: one JSON line, {"skipped": ...} or {name: [code, message]}"""
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

NEW = ("fa2_mla_indexer_logits_varlen", "fa2_topk_indices_varlen", "fa2_mla_indexer_topk_varlen", "fa2_mla_indexer_varlen_workspace_bytes")
IDX16 = 2
BF16, F16, F32, F64 = _lib.FA2_DTYPE_BF16, _lib.FA2_DTYPE_F16, _lib.FA2_DTYPE_F32, _lib.FA2_DTYPE_F64
E4M3, E5M2 = _lib.FA2_DTYPE_F8E4M3, _lib.FA2_DTYPE_F8E5M2
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
    for name in ("flash_attention_mla_indexer_topk_varlen", "mla_indexer_logits_varlen", "topk_indices_varlen", "check_mla_indexer_varlen_args"):
        assert name in fa.__all__ and callable(getattr(fa, name))
    assert _lib.mla_indexer_varlen_workspace_bytes(7, 2560) == 4 * 7 * 2560
    assert _lib.mla_indexer_varlen_workspace_bytes(1 << 20, 1 << 17) == 4 << 37  # (past 2^32)
    assert _lib.mla_indexer_varlen_workspace_bytes(1 << 28, 1 << 28) == 1 << 58
    assert _lib.mla_indexer_varlen_workspace_bytes(0, 5) == 0 and _lib.mla_indexer_varlen_workspace_bytes(1, 0) == 0
    # with B * N_q = total_q it is the fixed call's
    assert _lib.mla_indexer_varlen_workspace_bytes(6, 2560) == _lib.mla_indexer_workspace_bytes(3, 2, 2560)


def _i64(t):
    return None if t is None else (ctypes.c_int64 * len(t))(*t)


def _call(fn="topk", q=0x1000, w=0x2000, k=0x3000, ks=None, logits=0x4000, indices=0x5000, cu=0x8000, q_strides=NONE, w_strides=NONE,
          k_strides=NONE, ks_strides=NONE, logit_strides=NONE, index_strides=NONE, table=None, table_stride=NONE, B=3, H_I=64, total_q=7,
          max_q=4, S_k=512, num_blocks=32, page_size=64, max_blocks=8, d_I=128, dtype=BF16, k_dtype=None, causal=1, topk=200, variant=0):
    """fn: "logits" | "topk" (the fused call) | "select" (fa2_topk_indices_varlen).  Contiguous unless `table`; the cache in `dtype`
    unless `k_dtype`."""
    rows = page_size if table else S_k
    cap = max_blocks * page_size if table else S_k
    pick = lambda given, default: default if given is NONE else given
    qs = pick(q_strides, (max(H_I, 1) * d_I, d_I, 1))
    ws = pick(w_strides, (max(H_I, 1), 1))
    kst = pick(k_strides, (rows * d_I, d_I, 1))
    kss = pick(ks_strides, (rows, 1))
    lgs = pick(logit_strides, (cap, 1))
    ixs = pick(index_strides, (max(topk, 1), 1))
    l = _lib.lib()
    if fn == "select":
        rc = l.fa2_topk_indices_varlen(logits, _i64(lgs), cu, None, B, total_q, max_q, S_k, topk, causal, indices, _i64(ixs), None)
    else:
        head = (q, w, k, ks, logits, _i64(qs), _i64(ws), _i64(kst), _i64(kss), _i64(lgs), cu, None, table,
                pick(table_stride, max_blocks if table else 0), B, H_I, total_q, max_q, S_k, num_blocks, rows, max_blocks, d_I, dtype,
                dtype if k_dtype is None else k_dtype, causal)
        rc = l.fa2_mla_indexer_logits_varlen(*head, variant, None) if fn == "logits" else \
            l.fa2_mla_indexer_topk_varlen(*head, topk, indices, _i64(ixs), variant, None)
    return rc, l.fa2_last_error().decode()


PACKED = [  # what only the packed queries bring: all three entry points
    (dict(cu=None), -1, "varlen: null cu_seqlens_q"),
    (dict(total_q=0), -1, "varlen: total_q must be in [1, 2^28] (got 0)"), (dict(total_q=-2), -1, "varlen: total_q must be in [1, 2^28]"),
    (dict(total_q=(1 << 28) + 1), -1, "varlen: total_q must be in [1, 2^28]"),
    (dict(max_q=0), -1, "varlen: max_seqlen_q must be in [1, 2^28] (got 0)"), (dict(max_q=-1), -1, "varlen: max_seqlen_q must be in [1, 2^28]"),
    (dict(max_q=(1 << 28) + 1), -1, "varlen: max_seqlen_q must be in [1, 2^28]"),
    (dict(B=0), -1, "B must be in [1, 65535] (got 0)"), (dict(B=65536), -1, "B must be in [1, 65535]"),
    (dict(S_k=0), -1, "S_k must be in [1, 2^28]"), (dict(logits=None), -1, "null logits"), (dict(logit_strides=None), -1, "null logit_strides"),
    (dict(logit_strides=(-1, 1)), -1, "negative strides are not supported (logit_strides)"),
    (dict(logit_strides=(1, -1)), -1, "negative strides are not supported (logit_strides)"),
]
BOTH = [  # errors the scores bring: fa2_mla_indexer_logits_varlen and fa2_mla_indexer_topk_varlen alike
    (dict(q=None), -1, "mla indexer: null q_idx"), (dict(w=None), -1, "mla indexer: null weights"), (dict(k=None), -1, "mla indexer: null k_idx"),
    (dict(q_strides=None), -1, "null q_strides"), (dict(w_strides=None), -1, "null w_strides"), (dict(k_strides=None), -1, "null k_strides"),
    (dict(ks=0x6000, ks_strides=None), -1, "null k_scale_strides with a non-null k_scale"),
    (dict(q_strides=(-1, 1, 1)), -1, "negative strides are not supported (q_strides)"),
    (dict(q_strides=(1, 1, -1)), -1, "negative strides are not supported (q_strides)"),
    (dict(w_strides=(-1, 1)), -1, "negative strides are not supported (w_strides)"),
    (dict(w_strides=(1, -1)), -1, "negative strides are not supported (w_strides)"),
    (dict(k_strides=(1, -5, 1)), -1, "negative strides are not supported (k_strides)"),
    (dict(H_I=0), -1, "H_I must be >= 1 (got 0)"),
    (dict(table=0x7000, page_size=0), -1, "page_size"), (dict(table=0x7000, max_blocks=1 << 23), -1, "capacity"),
    (dict(table=0x7000, table_stride=-1), -1, "negative block_table_stride"),
    (dict(d_I=577), -2, "mla indexer: d_I=577 must be in [1, 576]"), (dict(dtype=F64), -2, "dtype_enum"), (dict(k_dtype=F16), -2, "k_dtype_enum"),
    (dict(k_dtype=E4M3), -1, "null k_scale with an fp8 cache"), (dict(k_dtype=E5M2), -1, "null k_scale with an fp8 cache"),
    (dict(k_dtype=E4M3, ks=0x6000, dtype=F32), -2, "goes with f16 / bf16 q_idx, not f32"),
    (dict(variant=3), -2, "mla indexer: unknown variant 3 (auto 0, generic 1, idx16 2)"),
    # a forced matrix form on what it cannot run
    (dict(variant=IDX16, dtype=F32), -2, "idx16 kernel: needs f16/bf16"), (dict(variant=IDX16, d_I=64), -2, "d_I = 128"),
    (dict(variant=IDX16, H_I=128), -2, "H_I <= 64"), (dict(variant=IDX16, k_strides=(512 * 256, 256, 2)), -2, "unit column strides"),
    (dict(variant=IDX16, q_strides=(64 * 132, 132, 1)), -2, "16-byte aligned rows"), (dict(variant=IDX16, k=0x3004), -2, "16-byte aligned rows"),
    # a grid that does not fit: key tiles * max_seqlen_q
    (dict(max_q=1 << 28, S_k=1 << 28), -1, "grid too large"), (dict(max_q=1 << 28, S_k=1 << 28, variant=1), -1, "grid too large"),
]
SELECT = [  # errors the selection brings: fa2_mla_indexer_topk_varlen and fa2_topk_indices_varlen alike
    (dict(indices=None), -1, "null indices"), (dict(index_strides=None), -1, "null index_strides"),
    (dict(index_strides=(200, -1)), -1, "negative strides are not supported (index_strides)"),
    (dict(index_strides=(-200, 1)), -1, "negative strides are not supported (index_strides)"),
    (dict(topk=0), -1, "topk must be in [1, 2^28] (got 0)"), (dict(topk=(1 << 28) + 1), -1, "topk must be in [1, 2^28]"),
]


@pytest.mark.parametrize("fn", ["logits", "topk", "select"])
@pytest.mark.parametrize("kwargs,code,needle", PACKED)
def test_packed_argument_errors_before_any_launch(fn, kwargs, code, needle):
    rc, msg = _call(fn, **kwargs)
    assert rc == code, (rc, msg)
    assert needle in msg, msg
    assert msg.startswith("topk indices" if fn == "select" else "mla indexer"), msg


@pytest.mark.parametrize("fn", ["logits", "topk"])
@pytest.mark.parametrize("kwargs,code,needle", BOTH)
def test_score_argument_errors_before_any_launch(fn, kwargs, code, needle):
    rc, msg = _call(fn, **kwargs)
    assert rc == code, (rc, msg)
    assert needle in msg, msg


@pytest.mark.parametrize("fn", ["topk", "select"])
@pytest.mark.parametrize("kwargs,code,needle", SELECT)
def test_selection_argument_errors_before_any_launch(fn, kwargs, code, needle):
    rc, msg = _call(fn, **kwargs)
    assert rc == code, (rc, msg)
    assert needle in msg, msg


def _forms():
    """the child: which kernel the first launch of a valid call is, read off the launch failure of a process without a device"""
    if torch.cuda.device_count() != 0:
        return {"skipped": "a device is visible"}
    out = {}
    fp8 = dict(k_dtype=E4M3, ks=0x6000)
    for name, kw in (("auto_h64", dict()), ("auto_h16", dict(H_I=16)), ("auto_h40", dict(H_I=40)), ("auto_f16", dict(dtype=F16)),
                     ("auto_fp8", fp8), ("auto_e5m2", dict(k_dtype=E5M2, ks=0x6000)), ("auto_scale", dict(ks=0x6000)),
                     ("auto_page1", dict(table=0x7000, page_size=1, max_blocks=512)), ("auto_page48", dict(table=0x7000, page_size=48)),
                     ("auto_page64", dict(table=0x7000)), ("auto_page48_fp8", dict(table=0x7000, page_size=48, **fp8)),
                     ("forced", dict(variant=IDX16)), ("auto_logits", dict(fn="logits")), ("forced_logits", dict(fn="logits", variant=IDX16)),
                     ("auto_f32", dict(dtype=F32)), ("auto_d64", dict(d_I=64)), ("auto_h128", dict(H_I=128)), ("generic", dict(variant=1)),
                     ("auto_colstride2", dict(k_strides=(512 * 256, 256, 2))), ("auto_unaligned", dict(k=0x3004)),
                     ("generic_logits", dict(fn="logits", variant=1)), ("select", dict(fn="select")),
                     ("forced_f32", dict(variant=IDX16, dtype=F32))):
        out[name] = list(_call(**kw))
    return out


def test_form_selection():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    run = subprocess.run([sys.executable, os.path.abspath(__file__), "--forms"], env=env, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    got = json.loads(run.stdout.strip().splitlines()[-1])
    if "skipped" in got:
        pytest.skip(got["skipped"])
    for name in ("auto_h64", "auto_h16", "auto_h40", "auto_f16", "auto_fp8", "auto_e5m2", "auto_scale", "auto_page1", "auto_page48", "auto_page64",
                 "auto_page48_fp8", "forced", "auto_logits", "forced_logits"):
        assert got[name][0] == -4 and "mla indexer idx16 kernel launch failed" in got[name][1], (name, got[name])
    for name in ("auto_f32", "auto_d64", "auto_h128", "generic", "auto_colstride2", "auto_unaligned", "generic_logits"):
        assert got[name][0] == -4 and "mla indexer generic kernel launch failed" in got[name][1], (name, got[name])
    assert got["select"][0] == -4 and "topk indices kernel launch failed" in got["select"][1], got["select"]
    assert got["forced_f32"][0] == -2 and "idx16 kernel: needs" in got["forced_f32"][1], got["forced_f32"]


def test_python_wrapper_errors():
    bf = torch.bfloat16
    q = torch.zeros(7, 64, 128, dtype=bf)
    w = torch.zeros(7, 64)
    k = torch.zeros(3, 256, 128, dtype=bf)
    cu = torch.tensor([0, 4, 4, 7], dtype=torch.int32)
    lens = torch.tensor([3, 100, 256], dtype=torch.int32)
    scale = torch.ones(3, 256)
    pool, table = torch.zeros(20, 48, 128, dtype=bf), torch.zeros(3, 6, dtype=torch.int32)

    def call(**kw):
        return fa.flash_attention_mla_indexer_topk_varlen(kw.pop("q", q), kw.pop("w", w), kw.pop("k", k), kw.pop("cu", cu), kw.pop("max_q", 4),
                                                          kw.pop("lens", lens), "cpu", **kw)

    for kw, needle in (
            (dict(q=q[0]), "q_idx must be"), (dict(q=[1]), "q_idx must be"), (dict(q=q[:, :, None]), "q_idx must be"),
            (dict(q=q.double()), "q_idx must be float16, bfloat16 or float32"),
            (dict(q=torch.zeros(7, 64, 600, dtype=bf), k=torch.zeros(3, 256, 600, dtype=bf)), "d_I in"),
            (dict(w=w.to(bf)), "weights must be"), (dict(w=w[:, :32]), "weights must be"), (dict(w=w[..., None]), "weights must be"),
            (dict(w=w[:6]), "weights must be"),
            (dict(cu=cu.long()), "cu_seqlens_q"), (dict(cu=cu[:1]), "cu_seqlens_q"), (dict(cu=[0, 7]), "cu_seqlens_q"),
            (dict(max_q=0), "max_seqlen_q"), (dict(max_q=4.0), "max_seqlen_q"), (dict(max_q=True), "max_seqlen_q"),
            (dict(k=k[0]), "k_idx must be"), (dict(k=k[..., :64]), "k_idx must be"), (dict(k=k[:2]), "k_idx must be"),
            (dict(k=k.float()), "k_idx must have q_idx's dtype"), (dict(k=k.to(torch.float8_e4m3fn)), "needs its k_scale"),
            (dict(k=k.float().to(torch.float8_e4m3fn), q=q.float(), k_scale=scale), "goes with float16 / bfloat16"),
            (dict(k_scale=scale[:, :100]), "k_scale must be"), (dict(k_scale=3.0), "k_scale must be"),
            (dict(lens=lens.long()), "cache_seqlens"), (dict(lens=lens[:2]), "cache_seqlens"),
            (dict(topk=0), "topk must be"), (dict(topk=2.0), "topk must be"), (dict(topk=True), "topk must be"),
            (dict(k=pool, block_table=table[:2]), "block_table"), (dict(k=pool, block_table=table.long()), "block_table"),
            (dict(variant="mla16"), "variant"), (dict(variant=2), "variant")):
        with pytest.raises(ValueError, match=needle):
            call(**kw)
    with pytest.raises(ValueError, match="dev="):
        fa.flash_attention_mla_indexer_topk_varlen(q, w, k, cu, 4, lens, "cuda:0")
    # what is fine reaches the launch, which refuses CPU tensors
    for kw in (dict(), dict(variant="idx16"), dict(variant="generic", topk=7), dict(lens=None), dict(causal=False, return_logits=True),
               dict(k_scale=scale), dict(k=k.to(torch.float8_e4m3fn), k_scale=scale), dict(k=pool, block_table=table),
               dict(q=q.float(), k=k.float()), dict(q=q[..., :64], k=k[..., :64]), dict(q=q.transpose(0, 1).contiguous().transpose(0, 1)),
               dict(max_q=1 << 28)):
        with pytest.raises(NotImplementedError):
            call(**kw)
    with pytest.raises(NotImplementedError):
        fa.mla_indexer_logits_varlen(q, w, k, cu, 4, lens, "cpu")
    with pytest.raises(ValueError, match="k_idx must be"):
        fa.mla_indexer_logits_varlen(q, w, k[0], cu, 4, lens, "cpu")
    lg = torch.zeros(7, 256)
    for kw, needle in ((dict(logits=lg.double()), "logits must be"), (dict(logits=lg[0]), "logits must be"), (dict(logits=lg[None]), "logits must be"),
                       (dict(topk=0), "topk must be"), (dict(cu=cu.long()), "cu_seqlens_q"), (dict(max_q=0), "max_seqlen_q"),
                       (dict(lens=lens[:2]), "cache_seqlens")):
        with pytest.raises(ValueError, match=needle):
            fa.topk_indices_varlen(kw.pop("logits", lg), kw.pop("cu", cu), kw.pop("max_q", 4), kw.pop("lens", lens), kw.pop("topk", 5), **kw)
    for kw in (dict(), dict(logits=lg[..., ::2]), dict(lens=None, causal=False)):
        with pytest.raises(NotImplementedError):
            fa.topk_indices_varlen(kw.pop("logits", lg), cu, 4, kw.pop("lens", lens), 5, **kw)
    # the pure check alone takes the same arguments
    fa.check_mla_indexer_varlen_args(q, w, k, cu, 4, lens)
    fa.check_mla_indexer_varlen_args(q, w, pool, cu, 4, None, 64, None, table)
    with pytest.raises(ValueError, match="topk"):
        fa.check_mla_indexer_varlen_args(q, w, k, cu, 4, lens, 0)


if __name__ == "__main__":
    if sys.argv[1:] != ["--forms"]:
        sys.exit(__doc__)
    print(json.dumps(_forms()))
