"""The fp8-query (_q8) entry points of the MLA indexer without a GPU; `--forms` is the child that sees no device (one JSON line)."""
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

NEW = ("fa2_mla_indexer_logits_q8", "fa2_mla_indexer_topk_q8", "fa2_mla_indexer_logits_varlen_q8", "fa2_mla_indexer_topk_varlen_q8")
IDX16, IDX8 = 2, 3
BF16, E4M3, E5M2 = _lib.FA2_DTYPE_BF16, _lib.FA2_DTYPE_F8E4M3, _lib.FA2_DTYPE_F8E5M2


def test_symbols_declared_bound_listed_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fa2_fwd.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exports = open(os.path.join(ROOT, "flash_attention_dlrs_amd", "csrc", "fa2_exports.map")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS
        assert re.search(rf"\b{name}\s*\(", header), name
        assert re.search(rf"\bT {name}\b", out), name
        assert re.search(rf"\b{name};", exports), name
        assert getattr(_lib.lib(), name).argtypes == getattr(_lib.lib(), name[:-3]).argtypes
    assert re.search(r"#define FA2_INDEXER_VARIANT_IDX8 3\b", header) and _lib.INDEXER_Q8_VARIANTS == {"auto": 0, "generic": 1, "idx8": 3}


_i64 = lambda t: (ctypes.c_int64 * len(t))(*t)  # noqa: E731


def _call(fn="topk", k=0x3000, ks=0x6000, k_strides=None, table=None, H_I=64, page_size=64, max_blocks=8, d_I=128,
          dtype=E4M3, k_dtype=E4M3, variant=0):
    B, N_q, S_k, topk, packed = 3, 2, 512, 200, fn.endswith("varlen")  # fake pointers; packed: total_q = 6
    rows, cap = (page_size, max_blocks * page_size) if table else (S_k, S_k)
    qs = (H_I * d_I, d_I, 1) if packed else (H_I * N_q * d_I, N_q * d_I, d_I, 1)
    ws, lgs, ixs = ((H_I, 1), (cap, 1), (topk, 1)) if packed else ((H_I * N_q, N_q, 1), (N_q * cap, cap, 1), (N_q * topk, topk, 1))
    head = [0x1000, 0x2000, k, ks, 0x4000, _i64(qs), _i64(ws), _i64(k_strides or (rows * d_I, d_I, 1)), _i64((rows, 1)), _i64(lgs)]
    head += [0x8000] if packed else []
    head += [None, table, max_blocks if table else 0, B, H_I] + ([B * N_q, N_q] if packed else [N_q])
    head += [S_k, 32, rows, max_blocks, d_I, dtype, k_dtype, 1]
    tail = [variant, None] if fn.startswith("logits") else [topk, 0x5000, _i64(ixs), variant, None]
    rc = getattr(_lib.lib(), f"fa2_mla_indexer_{fn}_q8")(*head, *tail)
    return rc, _lib.lib().fa2_last_error().decode()


@pytest.mark.parametrize("fn", ["logits", "topk", "logits_varlen", "topk_varlen"])
@pytest.mark.parametrize("kwargs,code,needle", [
    (dict(dtype=BF16), -2, "dtype_enum 2 (q_idx) must be FA2_DTYPE_F8E4M3 or FA2_DTYPE_F8E5M2"), (dict(dtype=99), -2, "dtype_enum 99 (q_idx)"),
    (dict(k_dtype=BF16), -2, "k_dtype_enum 2 must be FA2_DTYPE_F8E4M3 or FA2_DTYPE_F8E5M2"), (dict(dtype=E5M2, k_dtype=0), -2, "k_dtype_enum 0"),
    (dict(ks=None), -1, "null k_scale with an fp8 cache"),
    (dict(variant=IDX16), -2, "unknown variant 2 (auto 0, generic 1, idx8 3)"), (dict(variant=4), -2, "unknown variant 4 (auto 0, generic 1, idx8 3)"),
    (dict(variant=IDX8, d_I=64), -2, "idx8 kernel: needs fp8 q_idx and k_idx, d_I = 128"), (dict(variant=IDX8, H_I=128), -2, "H_I <= 64"),
    (dict(variant=IDX8, k_strides=(512 * 256, 256, 2)), -2, "unit column strides"),
    (dict(variant=IDX8, k_strides=(512 * 136, 136, 1)), -2, "16-byte aligned rows"), (dict(variant=IDX8, k=0x3004), -2, "16-byte aligned rows"),
])
def test_q8_argument_errors_before_any_launch(fn, kwargs, code, needle):
    rc, msg = _call(fn, **kwargs)
    assert rc == code and needle in msg, (rc, msg)


MATRIX = dict(e4m3_h64=dict(), e5m2_q=dict(dtype=E5M2), e5m2_k=dict(k_dtype=E5M2), e5m2_both=dict(dtype=E5M2, k_dtype=E5M2), h16=dict(H_I=16),
              h40=dict(H_I=40, dtype=E5M2), page1=dict(table=0x7000, page_size=1, max_blocks=512), page48=dict(table=0x7000, page_size=48),
              page64=dict(table=0x7000), forced=dict(variant=IDX8), logits=dict(fn="logits"), packed=dict(fn="topk_varlen"),
              packed_logits=dict(fn="logits_varlen", variant=IDX8))
VALU = dict(d64=dict(d_I=64), h128=dict(H_I=128), generic=dict(variant=1), colstride2=dict(k_strides=(512 * 256, 256, 2)),
            unaligned=dict(k=0x3004), packed_generic=dict(fn="topk_varlen", variant=1), packed_d64=dict(fn="logits_varlen", d_I=64))


def test_form_selection():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    run = subprocess.run([sys.executable, os.path.abspath(__file__), "--forms"], env=env, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    got = json.loads(run.stdout.strip().splitlines()[-1])
    if "skipped" in got:
        pytest.skip(got["skipped"])
    for name in MATRIX:
        assert got[name][0] == -4 and "mla indexer idx8 kernel launch failed" in got[name][1], (name, got[name])
    for name in VALU:
        assert got[name][0] == -4 and "mla indexer generic kernel launch failed" in got[name][1], (name, got[name])


def test_python_wrapper_errors():
    e4, bf = torch.float8_e4m3fn, torch.bfloat16
    q, w, k = torch.zeros(3, 64, 2, 128).to(e4), torch.zeros(3, 64, 2), torch.zeros(3, 256, 128).to(torch.float8_e5m2)
    lens, scale, cu = torch.tensor([3, 100, 256], dtype=torch.int32), torch.ones(3, 256), torch.tensor([0, 2, 4, 6], dtype=torch.int32)
    qp, wp = q.transpose(1, 2).reshape(6, 64, 128), torch.zeros(6, 64)
    fixed = lambda q=q, k=k, **kw: fa.flash_attention_mla_indexer_topk(q, w, k, lens, "cpu", k_scale=scale, **kw)  # noqa: E731
    packed = lambda q=qp, k=k, **kw: fa.flash_attention_mla_indexer_topk_varlen(q, wp, k, cu, 2, lens, "cpu", k_scale=scale, **kw)  # noqa: E731
    for call, q16 in ((fixed, q.to(bf)), (packed, qp.to(bf))):
        for kw, needle in ((dict(k=k.to(bf)), "k_idx must be float8_e4m3fn or float8_e5m2 under an fp8 q_idx"),
                           (dict(variant="idx16"), "variant 'idx16' does not go with an fp8 q_idx"),
                           (dict(q=q16, variant="idx8"), "variant 'idx8' does not go with a 16-bit or float32 q_idx"),
                           (dict(variant="mla16"), "variant must be one of")):
            with pytest.raises(ValueError, match=needle):
                call(**kw)
        for kw in (dict(), dict(variant="idx8"), dict(variant="generic"), dict(k=k.to(e4))):  # fine: the launch refuses CPU tensors
            with pytest.raises(NotImplementedError):
                call(**kw)


if __name__ == "__main__":
    print(json.dumps({"skipped": "a device is visible"} if torch.cuda.device_count() else
                     {name: list(_call(**kw)) for name, kw in {**MATRIX, **VALU}.items()}))
