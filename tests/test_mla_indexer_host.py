"""The MLA indexer (fa2_mla_indexer_logits, fa2_topk_indices, fa2_mla_indexer_topk, fa2_mla_indexer_workspace_bytes), the part that
needs no GPU: the four exported symbols, every argument error before any launch (fake pointers), which kernel a valid call launches
first (a child process that sees no device), the Python surface's errors on CPU tensors, quantize_index_keys, and the tie rule of
the restatement the GPU tests compare against.

    python tests/test_mla_indexer_host.py --forms     the child: one JSON line, {"skipped": ...} or {name: [code, message]}"""
import ctypes
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.join(ROOT, "tests")):
    if path not in sys.path:
        sys.path.insert(0, path)

import pytest
import torch

import flash_attention_dlrs_amd as fa
from flash_attention_dlrs_amd import _lib
from mla_indexer_restatement import counts, select_row, topk_lists

NEW = ("fa2_mla_indexer_logits", "fa2_topk_indices", "fa2_mla_indexer_topk", "fa2_mla_indexer_workspace_bytes")
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
    for name in ("flash_attention_mla_indexer_topk", "mla_indexer_logits", "topk_indices", "check_mla_indexer_args", "quantize_index_keys"):
        assert name in fa.__all__ and callable(getattr(fa, name))
    assert _lib.INDEXER_VARIANTS == {"auto": 0, "generic": 1, "idx16": 2}
    assert _lib.mla_indexer_workspace_bytes(3, 2, 2560) == 4 * 3 * 2 * 2560
    assert _lib.mla_indexer_workspace_bytes(128, 1024, 1 << 17) == 4 * 128 * 1024 * (1 << 17)  # (past 2^32)
    assert _lib.mla_indexer_workspace_bytes(65535, 1 << 28, 1 << 28) == (1 << 63) - 1  # does not fit: INT64_MAX
    assert _lib.mla_indexer_workspace_bytes(0, 2, 5) == 0 and _lib.mla_indexer_workspace_bytes(1, 1, 0) == 0


def _i64(t):
    return None if t is None else (ctypes.c_int64 * len(t))(*t)


def _call(fn="topk", q=0x1000, w=0x2000, k=0x3000, ks=None, logits=0x4000, indices=0x5000, q_strides=NONE, w_strides=NONE, k_strides=NONE,
          ks_strides=NONE, logit_strides=NONE, index_strides=NONE, table=None, table_stride=NONE, B=3, H_I=64, N_q=2, S_k=512,
          num_blocks=32, page_size=64, max_blocks=8, d_I=128, dtype=BF16, k_dtype=None, causal=1, topk=200, variant=0):
    """fn: "logits" | "topk" (the fused call) | "select" (fa2_topk_indices).  Contiguous unless `table`; the cache in `dtype` unless
    `k_dtype`."""
    rows = page_size if table else S_k
    cap = max_blocks * page_size if table else S_k
    pick = lambda given, default: default if given is NONE else given
    qs = pick(q_strides, (max(H_I, 1) * N_q * d_I, N_q * d_I, d_I, 1))
    ws = pick(w_strides, (max(H_I, 1) * N_q, N_q, 1))
    kst = pick(k_strides, (rows * d_I, d_I, 1))
    kss = pick(ks_strides, (rows, 1))
    lgs = pick(logit_strides, (N_q * cap, cap, 1))
    ixs = pick(index_strides, (N_q * max(topk, 1), max(topk, 1), 1))
    l = _lib.lib()
    if fn == "select":
        rc = l.fa2_topk_indices(logits, _i64(lgs), None, B, N_q, S_k, topk, causal, indices, _i64(ixs), None)
    else:
        head = (q, w, k, ks, logits, _i64(qs), _i64(ws), _i64(kst), _i64(kss), _i64(lgs), None, table,
                pick(table_stride, max_blocks if table else 0), B, H_I, N_q, S_k, num_blocks, rows, max_blocks, d_I, dtype,
                dtype if k_dtype is None else k_dtype, causal)
        rc = l.fa2_mla_indexer_logits(*head, variant, None) if fn == "logits" else \
            l.fa2_mla_indexer_topk(*head, topk, indices, _i64(ixs), variant, None)
    return rc, l.fa2_last_error().decode()


BOTH = [  # errors the scores bring: fa2_mla_indexer_logits and fa2_mla_indexer_topk alike
    (dict(q=None), -1, "mla indexer: null q_idx"), (dict(w=None), -1, "mla indexer: null weights"), (dict(k=None), -1, "mla indexer: null k_idx"),
    (dict(logits=None), -1, "mla indexer: null logits"), (dict(q_strides=None), -1, "null q_strides"), (dict(w_strides=None), -1, "null w_strides"),
    (dict(k_strides=None), -1, "null k_strides"), (dict(logit_strides=None), -1, "null logit_strides"),
    (dict(ks=0x6000, ks_strides=None), -1, "null k_scale_strides with a non-null k_scale"),
    (dict(q_strides=(1, 1, -1, 1)), -1, "negative strides are not supported (q_strides)"),
    (dict(w_strides=(-1, 1, 1)), -1, "negative strides are not supported (w_strides)"),
    (dict(k_strides=(1, -5, 1)), -1, "negative strides are not supported (k_strides)"),
    (dict(ks=0x6000, ks_strides=(1, -1)), -1, "negative strides are not supported (k_scale_strides)"),
    (dict(logit_strides=(1, 1, -1)), -1, "negative strides are not supported (logit_strides)"),
    (dict(B=0), -1, "B must be in [1, 65535] (got 0)"), (dict(B=65536), -1, "B must be in [1, 65535]"),
    (dict(H_I=0), -1, "H_I must be >= 1 (got 0)"), (dict(H_I=-4), -1, "H_I must be >= 1"),
    (dict(N_q=0), -1, "N_q must be in [1, 2^28]"), (dict(N_q=(1 << 28) + 1), -1, "N_q must be in [1, 2^28]"),
    (dict(S_k=0), -1, "S_k must be in [1, 2^28]"), (dict(S_k=(1 << 28) + 1), -1, "S_k must be in [1, 2^28]"),
    (dict(table=0x7000, page_size=0), -1, "page_size"), (dict(table=0x7000, num_blocks=0), -1, "num_blocks"),
    (dict(table=0x7000, max_blocks=1 << 23), -1, "capacity"), (dict(table=0x7000, table_stride=-1), -1, "negative block_table_stride"),
    (dict(d_I=0), -2, "mla indexer: d_I=0 must be in [1, 576]"), (dict(d_I=577), -2, "mla indexer: d_I=577 must be in [1, 576]"),
    (dict(dtype=F64), -2, "dtype_enum"), (dict(dtype=E4M3), -2, "dtype_enum"), (dict(dtype=99), -2, "dtype_enum"),
    (dict(k_dtype=F16), -2, "k_dtype_enum"), (dict(k_dtype=99, ks=0x6000), -2, "k_dtype_enum"),
    (dict(k_dtype=E4M3), -1, "null k_scale with an fp8 cache"), (dict(k_dtype=E5M2), -1, "null k_scale with an fp8 cache"),
    (dict(k_dtype=E4M3, ks=0x6000, dtype=F32), -2, "goes with f16 / bf16 q_idx, not f32"),
    (dict(variant=3), -2, "mla indexer: unknown variant 3 (auto 0, generic 1, idx16 2)"), (dict(variant=-1), -2, "unknown variant -1"),
    # a forced matrix form on what it cannot run
    (dict(variant=IDX16, dtype=F32), -2, "idx16 kernel: needs f16/bf16"), (dict(variant=IDX16, d_I=64), -2, "d_I = 128"),
    (dict(variant=IDX16, H_I=128), -2, "H_I <= 64"), (dict(variant=IDX16, k_strides=(512 * 256, 256, 2)), -2, "unit column strides"),
    (dict(variant=IDX16, q_strides=(64 * 2 * 132, 2 * 132, 132, 1)), -2, "16-byte aligned rows"),
    (dict(variant=IDX16, k=0x3004), -2, "16-byte aligned rows"),
    (dict(variant=IDX16, k_dtype=E4M3, ks=0x6000, k_strides=(512 * 136, 136, 1)), -2, "16-byte aligned rows"),
    # a grid that does not fit: key tiles * N_q
    (dict(N_q=1 << 28, S_k=1 << 28), -1, "grid too large"), (dict(N_q=1 << 28, S_k=1 << 28, variant=1), -1, "grid too large"),
]
SELECT = [  # errors the selection brings: fa2_mla_indexer_topk and fa2_topk_indices alike
    (dict(indices=None), -1, "null indices"), (dict(index_strides=None), -1, "null index_strides"),
    (dict(index_strides=(400, 200, -1)), -1, "negative strides are not supported (index_strides)"),
    (dict(topk=0), -1, "topk must be in [1, 2^28] (got 0)"), (dict(topk=-3), -1, "topk must be in [1, 2^28]"),
    (dict(topk=(1 << 28) + 1), -1, "topk must be in [1, 2^28]"),
    (dict(logits=None), -1, "null logits"), (dict(logit_strides=None), -1, "null logit_strides"),
    (dict(logit_strides=(-1, 1, 1)), -1, "negative strides are not supported (logit_strides)"),
    (dict(B=0), -1, "B must be in [1, 65535]"), (dict(N_q=0), -1, "N_q must be in [1, 2^28]"), (dict(S_k=0), -1, "S_k must be in [1, 2^28]"),
    (dict(B=65535, N_q=1 << 20, S_k=64), -1, "grid too large (B * N_q"),
]


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
    assert msg.startswith("topk indices" if fn == "select" else "mla indexer"), msg


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
    q = torch.zeros(3, 64, 2, 128, dtype=bf)
    w = torch.zeros(3, 64, 2)
    k = torch.zeros(3, 256, 128, dtype=bf)
    lens = torch.tensor([3, 100, 256], dtype=torch.int32)
    scale = torch.ones(3, 256)
    pool, table = torch.zeros(20, 48, 128, dtype=bf), torch.zeros(3, 6, dtype=torch.int32)

    def call(**kw):
        return fa.flash_attention_mla_indexer_topk(kw.pop("q", q), kw.pop("w", w), kw.pop("k", k), kw.pop("lens", lens), "cpu", **kw)

    for kw, needle in (
            (dict(q=q[0]), "q_idx must be"), (dict(q=[1]), "q_idx must be"), (dict(q=q.double()), "q_idx must be float16, bfloat16 or float32"),
            (dict(q=torch.zeros(3, 64, 2, 600, dtype=bf), k=torch.zeros(3, 256, 600, dtype=bf)), "d_I in"),
            (dict(w=w.to(bf)), "weights must be"), (dict(w=w[:, :32]), "weights must be"), (dict(w=w[..., None]), "weights must be"),
            (dict(k=k[0]), "k_idx must be"), (dict(k=k[..., :64]), "k_idx must be"), (dict(k=k[:2]), "k_idx must be"),
            (dict(k=k.float()), "k_idx must have q_idx's dtype"), (dict(k=k.to(torch.float8_e4m3fn)), "needs its k_scale"),
            (dict(k=k.to(torch.float8_e5m2)), "needs its k_scale"),
            (dict(k=k.float().to(torch.float8_e4m3fn), q=q.float(), k_scale=scale), "goes with float16 / bfloat16"),
            (dict(k_scale=scale[:, :100]), "k_scale must be"), (dict(k_scale=scale.double()), "k_scale must be"), (dict(k_scale=3.0), "k_scale must be"),
            (dict(lens=lens.long()), "cache_seqlens"), (dict(lens=lens[:2]), "cache_seqlens"),
            (dict(topk=0), "topk must be"), (dict(topk=2.0), "topk must be"), (dict(topk=True), "topk must be"), (dict(topk=(1 << 28) + 1), "topk must be"),
            (dict(k=pool, block_table=table[:2]), "block_table"), (dict(k=pool, block_table=table.long()), "block_table"),
            (dict(variant="mla16"), "variant"), (dict(variant=2), "variant")):
        with pytest.raises(ValueError, match=needle):
            call(**kw)
    with pytest.raises(ValueError, match="dev="):
        fa.flash_attention_mla_indexer_topk(q, w, k, lens, "cuda:0")
    # what is fine reaches the launch, which refuses CPU tensors
    for kw in (dict(), dict(variant="idx16"), dict(variant="generic", topk=7), dict(lens=None), dict(causal=False, return_logits=True),
               dict(k_scale=scale), dict(k=k.to(torch.float8_e4m3fn), k_scale=scale), dict(k=pool, block_table=table),
               dict(q=q.float(), k=k.float()), dict(q=q[..., :64], k=k[..., :64]), dict(q=q.transpose(1, 2).contiguous().transpose(1, 2))):
        with pytest.raises(NotImplementedError):
            call(**kw)
    with pytest.raises(NotImplementedError):
        fa.mla_indexer_logits(q, w, k, lens, "cpu")
    with pytest.raises(ValueError, match="k_idx must be"):
        fa.mla_indexer_logits(q, w, k[0], lens, "cpu")
    lg = torch.zeros(3, 2, 256)
    for kw, needle in ((dict(logits=lg.double()), "logits must be"), (dict(logits=lg[0, 0]), "logits must be"), (dict(topk=0), "topk must be"),
                       (dict(N_q=3), "N_q"), (dict(logits=lg.flatten(0, 1)), "need N_q"), (dict(logits=lg.flatten(0, 1), N_q=4), "need N_q"),
                       (dict(lens=lens[:2]), "cache_seqlens")):
        with pytest.raises(ValueError, match=needle):
            fa.topk_indices(kw.pop("logits", lg), kw.pop("lens", lens), kw.pop("topk", 5), **kw)
    for kw in (dict(), dict(N_q=2), dict(logits=lg.flatten(0, 1), N_q=2), dict(logits=lg[..., ::2]), dict(lens=None, causal=False)):
        with pytest.raises(NotImplementedError):
            fa.topk_indices(kw.pop("logits", lg), kw.pop("lens", lens), 5, **kw)
    # the pure check alone takes the same arguments
    fa.check_mla_indexer_args(q, w, k, lens)
    fa.check_mla_indexer_args(q, w, pool, None, 64, None, table)
    with pytest.raises(ValueError, match="topk"):
        fa.check_mla_indexer_args(q, w, k, lens, 0)


@pytest.mark.parametrize("dtype", [torch.float8_e4m3fn, torch.float8_e5m2])
def test_quantize_index_keys_round_trips_exactly(dtype):
    g = torch.Generator().manual_seed(3)
    k = torch.randn(4, 50, 128, generator=g) * torch.logspace(-6, 6, 50)[None, :, None]
    k[0, 0] = 0  # a row of zeros: scale 1
    k[1, 1] = torch.finfo(dtype).max * 4.0  # amax / scale == the format's largest value exactly
    k8, s = fa.quantize_index_keys(k.to(torch.bfloat16), dtype)
    assert k8.dtype == dtype and k8.shape == k.shape and s.dtype == torch.float32 and s.shape == (4, 50)
    m, _ = torch.frexp(s)
    assert (m == 0.5).all() and s[0, 0] == 1 and s[1, 1] == 4  # powers of two
    top = torch.finfo(dtype).max
    amax = k.to(torch.bfloat16).float().abs().amax(-1)
    assert (amax / s <= top).all() and ((amax / s > top / 2) | (amax == 0)).all()  # the smallest such power
    assert not torch.isnan(k8.float()).any() and (k8.float().abs() <= top).all()
    deq = k8.float() * s[..., None]
    again8, again_s = fa.quantize_index_keys(deq, dtype)  # quantising what was dequantised changes nothing
    assert torch.equal(again8.float() * again_s[..., None], deq)
    # a value the format holds exactly at the row's scale comes back exactly
    exact = torch.tensor([[1.0, -2.0, 0.5, 1.75, 0.0, -0.25, 448.0 if dtype == torch.float8_e4m3fn else 57344.0, 3.0]])
    e8, es = fa.quantize_index_keys(exact, dtype)
    assert torch.equal(e8.float() * es[..., None], exact)
    with pytest.raises(ValueError, match="dtype"):
        fa.quantize_index_keys(k, torch.float16)


INF, NAN = float("inf"), float("nan")


@pytest.mark.parametrize("row,topk,want", [
    ([5.0] * 6, 3, [0, 1, 2]),                                   # all equal: the lowest positions
    ([0.0, -0.0, 0.0, -0.0, -1.0], 3, [0, 1, 2]),               # -0.0 == +0.0: position decides
    ([-0.0, 0.0, 1.0], 2, [0, 2]),
    ([1.0, NAN, 3.0, 2.0], 2, [2, 3]),                           # a NaN ranks as -inf
    ([NAN, -INF, NAN, -INF, 0.0], 3, [0, 1, 4]),                 # ... and ties with it by position
    ([-INF, -5.0, -INF, INF], 3, [0, 1, 3]),
    ([3.0, 1.0, 2.0], 5, [0, 1, 2, -1, -1]),                     # n < topk: the identity, padded
    ([3.0, 1.0, 2.0], 3, [0, 1, 2]),                             # n == topk
    ([3.0, 1.0, 2.0, 1.0], 3, [0, 1, 2]),                        # n == topk + 1: one leaves, the later of the tie
    ([1.0, 3.0, 1.0, 2.0], 3, [0, 1, 3]),
    ([2.0, 1.0, 2.0, 1.0, 2.0, 1.0], 4, [0, 1, 2, 4]),           # emitted in ascending position, not by value
    ([], 2, [-1, -1]),
])
def test_restatement_tie_rule_on_hand_written_rows(row, topk, want):
    assert select_row(torch.tensor(row, dtype=torch.float32), topk) == want


def test_restatement_candidates_and_rows():
    assert counts([0, 1, 5, 9], 4, 3, 5, True) == [[0, 0, 0], [0, 0, 1], [3, 4, 5], [3, 4, 5]]  # (9 clamps to S_k = 5)
    assert counts([0, 1, 5], 3, 3, 5, False) == [[0, 0, 0], [1, 1, 1], [5, 5, 5]] and counts(None, 1, 2, 4, True) == [[3, 4]]
    lg = torch.tensor([[[1.0, 9.0, 9.0, NAN, INF], [1.0, 9.0, 9.0, 7.0, INF]]])
    # sequence of 4 keys, two queries: the first sees keys 0..2, the second 0..3; entry 4 is no candidate whatever it holds
    assert topk_lists(lg, [4], 2, True).tolist() == [[[1, 2], [1, 2]]]
    assert topk_lists(lg, [4], 3, False).tolist() == [[[0, 1, 2], [1, 2, 3]]]
    assert topk_lists(lg, None, 1, False).tolist() == [[[4], [4]]]


if __name__ == "__main__":
    if sys.argv[1:] != ["--forms"]:
        sys.exit(__doc__)
    print(json.dumps(_forms()))
