"""Dense MLA decode over the tile-scaled fp8 cache (fa2_fwd_kvcache_mla_ds, _varlen_ds; kv_format="fp8_ds" of the two dense latent calls)
without a GPU: symbols, codes and messages (fake pointers), the first kernel of a valid call (--forms: a child that sees no device),
wrapper errors."""
import ctypes
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import pytest
import torch

import flash_attention_dlrs_amd as fa
from flash_attention_dlrs_amd import _lib

NEW = ("fa2_fwd_kvcache_mla_ds", "fa2_fwd_kvcache_mla_varlen_ds")
BF16, F32 = _lib.FA2_DTYPE_BF16, _lib.FA2_DTYPE_F32


def test_symbols_declared_bound_listed_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fa2_fwd.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exports = open(os.path.join(ROOT, "flash_attention_dlrs_amd", "csrc", "fa2_exports.map")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS and re.search(rf"\b{name}\s*\(", header) and re.search(rf"\bT {name}\b", out), name
        assert re.search(rf"\b{name};", exports) and getattr(_lib.lib(), name).argtypes is not None and callable(getattr(_lib, name)), name


def _call(packed=False, kv=0x1000, row=656, page=0, dtype=BF16, variant=0, kv_strides=True, B=3, H=16, N_q=2, S_k=512):
    """one call on fake pointers: a contiguous cache of S_k keys or, with page, a pool of 24 pages behind a table of 8 entries a row"""
    i64 = lambda t: None if t is None else (ctypes.c_int64 * len(t))(*t)
    rows = page or S_k
    kvs = i64((rows * row, rows * row, row)) if kv_strides else None
    table = (0x5000, 8) if page else (None, 0)
    tail = (dtype, 1, 1.0, -1, -1, 1, None, 0, variant, None)
    if packed:
        rc = _lib.lib().fa2_fwd_kvcache_mla_varlen_ds(
            0x1000, kv, 0x1000, 0x1000, i64((H * 576, 576, 1)), kvs, i64((H * 512, 512, 1)), B * N_q, 0x6000, None, *table,
            B, H, 1, B * N_q, N_q, 0 if page else S_k, 24 if page else 0, page, 8 if page else 0, *tail)
    else:
        rc = _lib.lib().fa2_fwd_kvcache_mla_ds(
            0x1000, kv, 0x1000, 0x1000, i64((H * N_q * 576, N_q * 576, 576, 1)), kvs, i64((H * N_q * 512, N_q * 512, 512, 1)),
            i64((H * N_q, N_q)), None, *table, B, H, 1, N_q, 24 if page else 0, page or S_k, 8 if page else 0, *tail)
    return rc, _lib.lib().fa2_last_error().decode()


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("kwargs,code,needle", [
    (dict(kv=None), -1, "kvcache mla fp8_ds: null KV"), (dict(kv_strides=False), -1, "kvcache mla fp8_ds: null kv_strides"),
    (dict(row=-656), -1, "kvcache mla fp8_ds: negative strides are not supported (kv_strides, in bytes)"),
    (dict(dtype=F32), -2, "kvcache mla fp8_ds: dtype_enum"), (dict(variant=2), -2, "kvcache mla fp8_ds: unknown variant 2"),
    (dict(variant=3, row=660), -2, "multiples of 16 bytes"), (dict(variant=3, kv=0x1004), -2, "fp8_ds cache: needs"),
    (dict(variant=3, page=16), -2, "page_size % 64 == 0"),
])
def test_argument_errors_before_any_launch(kwargs, code, needle, packed):
    rc, msg = _call(packed, **kwargs)
    assert rc == code and needle in msg, (rc, msg)


MATRIX = ("aligned", "forced", "page64")


def _forms():
    if torch.cuda.device_count() != 0:
        return {"skipped": "a device is visible"}
    cases = (("aligned", dict()), ("forced", dict(variant=3)), ("page64", dict(page=64)), ("page16", dict(page=16)), ("base4", dict(kv=0x1004)),
             ("row660", dict(row=660)), ("generic", dict(variant=1)))
    return {f"{name}{int(p)}": list(_call(p, **kw)) for name, kw in cases for p in (False, True)}


def test_form_selection():
    run = subprocess.run([sys.executable, os.path.abspath(__file__), "--forms"], env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"),
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    got = json.loads(run.stdout.strip().splitlines()[-1])
    if "skipped" in got:
        pytest.skip(got["skipped"])
    for name, (rc, msg) in got.items():
        want = "kvcache mla16 kernel launch failed" if name[:-1] in MATRIX else "kvcache generic kernel launch failed"
        assert rc == -4 and want in msg, (name, rc, msg)


def test_python_wrapper_errors():
    bf = torch.bfloat16
    Q, KV = torch.zeros(3, 16, 2, 576, dtype=bf), torch.zeros(3, 1, 128, 656, dtype=torch.uint8)
    lens, cu = torch.tensor([3, 100, 128], dtype=torch.int32), torch.tensor([0, 2, 3, 6], dtype=torch.int32)

    def fixed(**kw):
        return fa.flash_attention_mla_decode_forward(kw.pop("Q", Q), kw.pop("KV", KV), lens, "cpu", **{"kv_format": "fp8_ds", **kw})

    def packed(**kw):
        q = kw.pop("Q", Q).transpose(1, 2).flatten(0, 1)
        if "kv_new" in kw:
            kw["kv_new"] = kw["kv_new"].transpose(1, 2).flatten(0, 1)
        return fa.flash_attention_mla_varlen_decode_forward(q, kw.pop("KV", KV), cu, 3, lens, "cpu", **{"kv_format": "fp8_ds", **kw})

    for call in (fixed, packed):
        for kw, needle in ((dict(kv_format="fp8"), "kv_format must be"), (dict(KV=KV.view(torch.int8)), "torch.uint8"),
                           (dict(KV=KV[..., :576]), "656 bytes"), (dict(Q=Q.float()), "float16 / bfloat16"), (dict(d_v=256), "d_v = 512"),
                           (dict(kv_descale=torch.ones(3, 1)), "no kv_descale"), (dict(KV=KV[:2]), "kvcache"),
                           (dict(kv_new=torch.zeros(3, 1, 2, 576, dtype=bf)), r"mla_kvcache_append\(\.\.\., kv_format=\"fp8_ds\"\)"),
                           (dict(variant="mfma16"), "variant must be")):
            with pytest.raises(ValueError, match=needle):
                call(**kw)
        with pytest.raises(NotImplementedError):  # what is fine (a misaligned view, causal, a window) reaches the launch, which refuses CPU tensors
            call(KV=torch.zeros(3, 1, 128, 660, dtype=torch.uint8)[..., 4:], Q=Q.half(), causal=True, window=(64, 0))


if __name__ == "__main__":
    print(json.dumps(_forms()))
