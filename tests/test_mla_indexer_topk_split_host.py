"""The split-row selection of the MLA indexer (fa2_topk_indices_split, fa2_topk_indices_varlen_split, fa2_topk_workspace_bytes,
fa2_topk_num_splits), the part that needs no GPU: the four symbols, the argument errors before any launch (fake pointers), the
workspace formula, the heuristic's conditions, the Python surface's errors on CPU tensors."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import flash_attention_dlrs_amd as fa
from flash_attention_dlrs_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fa2_topk_indices_split", "fa2_topk_indices_varlen_split", "fa2_topk_workspace_bytes", "fa2_topk_num_splits")


def test_symbols_declared_bound_listed_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fa2_fwd.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exports = open(os.path.join(ROOT, "flash_attention_dlrs_amd", "csrc", "fa2_exports.map")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS and re.search(rf"\b{name}\s*\(", header) and re.search(rf"\bT {name}\b", out), name
        assert re.search(rf"\b{name};", exports) and getattr(_lib.lib(), name).argtypes is not None, name


def _i64(t):
    return None if t is None else (ctypes.c_int64 * len(t))(*t)


def _call(packed=False, logits=0x4000, indices=0x5000, B=3, N_q=2, S_k=3000, topk=200, index_strides=(400, 200, 1), num_splits=2,
          workspace=0x8000, workspace_bytes=1 << 30):
    l = _lib.lib()
    if packed:
        rc = l.fa2_topk_indices_varlen_split(logits, _i64((S_k, 1)), 0x6000, None, B, B * N_q, N_q, S_k, topk, 1, indices,
                                             _i64(index_strides[1:]), num_splits, workspace, workspace_bytes, None)
    else:
        rc = l.fa2_topk_indices_split(logits, _i64((N_q * S_k, S_k, 1)), None, B, N_q, S_k, topk, 1, indices, _i64(index_strides),
                                      num_splits, workspace, workspace_bytes, None)
    return rc, l.fa2_last_error().decode()


NEED = 6 * (4 * 5120 + 8 * 2)  # six rows at two splits


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("kwargs,needle", [
    (dict(num_splits=-1), "num_splits must be in [0, 256] (got -1)"), (dict(num_splits=257), "num_splits must be in [0, 256] (got 257)"),
    (dict(workspace=None), "null workspace"), (dict(workspace=0x8004), "workspace must be 16-byte aligned"),
    (dict(workspace_bytes=NEED - 1), f"workspace_bytes = {NEED - 1} is short of the {NEED} bytes"),
    (dict(num_splits=256, workspace_bytes=6 * (4 * 5120 + 8 * 3) - 1), "is short of"),  # (256 clamps to the 3 chunks of 3,000 keys)
    (dict(B=65535, N_q=2, workspace_bytes=1 << 40), "grid too large for num_splits = 2"),
    # the checks of fa2_topk_indices come first
    (dict(num_splits=-1, indices=None), "null indices"), (dict(workspace=None, topk=0), "topk must be in [1, 2^28]"),
    (dict(num_splits=999, S_k=0), "S_k must be in [1, 2^28]"), (dict(workspace=None, index_strides=(400, 200, -1)), "negative strides"),
])
def test_split_argument_errors_before_any_launch(packed, kwargs, needle):
    rc, msg = _call(packed, **kwargs)
    assert rc == -1 and needle in msg and msg.startswith("topk indices"), (rc, msg)


@pytest.mark.skipif(torch.cuda.device_count() != 0, reason="a device is visible: a valid call would launch on fake pointers")
@pytest.mark.parametrize("kwargs,kernel", [
    (dict(workspace_bytes=NEED), "topk indices split kernel"), (dict(num_splits=1, workspace=None, workspace_bytes=0), "topk indices kernel"),
    (dict(num_splits=0, workspace=None, workspace_bytes=0), "topk indices kernel"),  # (the heuristic: 1 below 8,192 keys)
    (dict(S_k=1024, workspace=None, workspace_bytes=0), "topk indices kernel"),  # (one chunk: no split, no workspace)
])
def test_which_kernel_a_valid_call_launches(kwargs, kernel):
    for packed in (False, True):
        rc, msg = _call(packed, **kwargs)
        assert rc == -4 and f"{kernel} launch failed" in msg, (rc, msg)


def test_workspace_bytes_and_heuristic():
    ws, ns = _lib.topk_workspace_bytes, _lib.topk_num_splits
    assert [ws(1, 2), ws(6, 2), ws(7, 256), ws(1 << 20, 64)] == [r * (4 * (2048 + 2048 + 1024) + 8 * s)
                                                                 for r, s in ((1, 2), (6, 2), (7, 256), (1 << 20, 64))]
    assert ws(0, 2) == 0 and ws(5, 1) == 0 and ws(5, 0) == 0 and ws(5, 257) == 0
    sizes = (1, 1000, 8191, 8192, 8193, 16384, 65536, 163840, 1 << 28)
    for S_k in sizes:
        last = 256
        for rows in (1, 2, 3, 16, 32, 128, 255, 256, 1024, 65535, 1 << 28):
            got = ns(rows, S_k, 2048)
            assert 1 <= got <= min(last, 256), (rows, S_k, got)  # non-increasing in rows
            assert got == 1 if S_k < 8192 or rows >= 256 else got > 1, (rows, S_k, got)
            assert got <= max(1, -(-S_k // 1024)), (rows, S_k, got)  # every chunk of 1,024 positions at least holds one
            last = got
    assert all(ns(1, S_k, 2048) == 1 for S_k in range(1, 8192, 97)) and ns(1, 16384, 16384) == 1 and ns(0, 65536, 2048) == 1


def test_python_wrapper_errors():
    lg, lens, cu = torch.zeros(3, 2, 256), torch.tensor([3, 100, 256], dtype=torch.int32), torch.tensor([0, 2, 4, 6], dtype=torch.int32)
    q, w, k = torch.zeros(3, 64, 2, 128, dtype=torch.bfloat16), torch.zeros(3, 64, 2), torch.zeros(3, 256, 128, dtype=torch.bfloat16)
    qp, wp = q.transpose(1, 2).flatten(0, 1), w.transpose(1, 2).flatten(0, 1)
    for bad in (-1, 257, 2.0, True, None):
        with pytest.raises(ValueError, match="num_splits must be an int in"):
            fa.topk_indices(lg, lens, 5, num_splits=bad)
        with pytest.raises(ValueError, match="num_splits must be an int in"):
            fa.topk_indices_varlen(lg.flatten(0, 1), cu, 2, lens, 5, num_splits=bad)
        with pytest.raises(ValueError, match="select_splits must be an int in"):
            fa.flash_attention_mla_indexer_topk(q, w, k, lens, "cpu", select_splits=bad)
        with pytest.raises(ValueError, match="select_splits must be an int in"):
            fa.flash_attention_mla_indexer_topk_varlen(qp, wp, k, cu, 2, lens, "cpu", select_splits=bad)
    for count in (0, 1):  # what is fine reaches the launch, which refuses CPU tensors
        with pytest.raises(NotImplementedError):
            fa.topk_indices(lg, lens, 5, num_splits=count)
        with pytest.raises(NotImplementedError):
            fa.flash_attention_mla_indexer_topk_varlen(qp, wp, k, cu, 2, lens, "cpu", select_splits=count)
