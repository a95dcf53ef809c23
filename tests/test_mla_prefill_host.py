"""The packed forward with a value head size of its own (fa2_fwd_varlen_dv, fa2_fwd_varlen_dv_variant), the part that needs no GPU:
the two exported symbols and the variant table, every argument error before any launch and which kernel a valid call launches
first (fake pointers, in a child process that sees no device), and the Python surface's errors on CPU tensors.

    python tests/test_mla_prefill_host.py --calls     the child: one JSON line, {"skipped": ...} or {name: [code, message]}"""
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
from flash_attention_dlrs_amd import flash_attention_torch as T

NEW = ("fa2_fwd_varlen_dv", "fa2_fwd_varlen_dv_variant")
MFMA16DV = 28
F32, F16, BF16, F8E5, F8E4, F64 = range(6)


def test_symbols_declared_bound_exported_and_listed():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fa2_fwd.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exports = open(os.path.join(ROOT, "flash_attention_dlrs_amd", "csrc", "fa2_exports.map")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS
        assert re.search(rf"\b{name}\s*\(", header), name
        assert re.search(rf"\bT {name}\b", out), name
        assert re.search(rf"\b{name};", exports), name
        assert getattr(_lib.lib(), name).argtypes is not None
    assert re.search(r"#define\s+FA2_VARIANT_MFMA16DV\s+28\b", header)
    assert "flash_attention_mla_prefill_forward" in fa.__all__ and callable(fa.flash_attention_mla_prefill_forward)
    assert callable(_lib.fa2_fwd_varlen_dv) and callable(T.check_varlen_dv_args)


def test_variant_tables():
    assert _lib.VARLEN_DV_VARIANTS == {"auto": 0, "generic": 1, "mfma16dv": MFMA16DV}
    # an id no other constant uses, the experimental ones included; nothing renumbered
    assert MFMA16DV not in _lib.VARIANTS.values() and MFMA16DV not in _lib.EXPERIMENTAL_VARIANTS.values()
    published = {"auto": 0, "generic": 1, "mfma16": 2, "mfma16_w8": 3, "mfma32": 4, "mfma16d": 8, "mfma16d_w4": 9, "mfma16h": 14,
                 "mfma16h_w4": 15, "mfma8x": 16, "mfma8x_w4": 17, "mfma16k": 19, "mfma16k_r2k2": 20, "mfma16k_r2k4": 23, "a64": 24,
                 "a16": 25, "a8": 26, "a64d": 27}
    assert {k: v for k, v in _lib.VARIANTS.items() if k not in _lib.EXPERIMENTAL_VARIANTS} == published
    assert _lib.BWD_VARIANTS == {"auto": 0, "generic": 1, "mfma16": 2, "mfma32": 3}
    assert _lib.KVCACHE_VARIANTS == {"auto": 0, "generic": 1, "mfma16": 2}
    assert _lib.KVCACHE_MLA_VARIANTS == {"auto": 0, "generic": 1, "mla16": 3}


def _call(ptr=0x1000, nulls=(), cu=0x3000, B=3, H=16, H_kv=16, d=192, d_v=128, total=700, max_len=300, dtype=BF16, variant=0, scale=0.07,
          window=(-1, -1), q_strides=None, k_strides=None, v_strides=None, o_strides=None, plain=False):
    """a contiguous packed call on fake pointers -> (code, message; a launch failure's ends at "launch failed")"""
    i64 = lambda v: (ctypes.c_int64 * len(v))(*v)
    t = {n: (None if n in nulls else ptr) for n in "QKVOL"}
    qs, ks = q_strides or (H * d, d, 1), k_strides or (H_kv * d, d, 1)
    w = d_v if d_v > 0 else 128  # (a d_v that is refused still comes with usable strides)
    vs, os_ = v_strides or (H_kv * w, w, 1), o_strides or (H * w, w, 1)
    args = [t["Q"], t["K"], t["V"], t["O"], t["L"], i64(qs), i64(ks), i64(vs), i64(os_), total, cu, cu, B, H, H_kv, d, d_v, max_len,
            max_len, total, total, dtype, 1, scale, window[0], window[1], None]
    lib = _lib.lib()
    rc = lib.fa2_fwd_varlen_dv(*args) if plain else lib.fa2_fwd_varlen_dv_variant(*args, variant)
    msg = lib.fa2_last_error().decode()
    cut = msg.find("launch failed")
    return [rc, msg if cut < 0 else msg[:cut + len("launch failed")]]


ERRORS = [  # (name, arguments, code, what the message must hold)
    ("d_v_0", dict(d_v=0), -1, "d_v=0 must be in [1, 512]"), ("d_v_513", dict(d_v=513), -1, "d_v=513 must be in [1, 512]"),
    ("d_v_neg", dict(d_v=-128), -1, "d_v"),
    ("d_513", dict(d=513), -2, "d=513 must be in [1, 512]"), ("d_0", dict(d=0), -1, "d=0"),       # as fa2_fwd_varlen_gqa answers
    ("gqa", dict(H=16, H_kv=3), -1, "H_kv must divide H"), ("h_kv_0", dict(H_kv=0), -1, "H_kv"),
    ("neg_stride", dict(v_strides=(2048, -128, 1)), -1, "negative strides"),
    ("null_V", dict(nulls="V"), -1, "varlen: null V"), ("null_O", dict(nulls="O"), -1, "varlen: null O"),
    ("null_cu", dict(cu=None), -1, "null cu_seqlens_q"),
    ("fp8_e4m3", dict(dtype=F8E4), -2, "fp8 is not supported"), ("fp8_e5m2", dict(dtype=F8E5), -2, "fp8 is not supported"),
    ("B_0", dict(B=0), -1, "B (number of sequences)"), ("window", dict(window=(-2, 0)), -1, "window"),
    ("scale_nan", dict(scale=float("nan")), -1, "NaN"),
    # the order is fa2_fwd_varlen_gqa's, d_v last
    ("gqa_before_d_v", dict(H_kv=3, d_v=0), -1, "H_kv"), ("fp8_before_d_v", dict(dtype=F8E4, d_v=0), -2, "fp8"),
    ("stride_before_d_v", dict(q_strides=(-1, 192, 1), d_v=0), -1, "negative strides"),
    # a forced matrix kernel on what it cannot take, and what is no variant of this call
    ("forced_128_128", dict(variant=MFMA16DV, d=128, d_v=128), -2, "mfma16dv kernel: needs"),
    ("forced_192_192", dict(variant=MFMA16DV, d=192, d_v=192), -2, "d = 192 and d_v = 128"),
    ("forced_f32", dict(variant=MFMA16DV, dtype=F32), -2, "f16/bf16"),
    ("forced_dstride2", dict(variant=MFMA16DV, k_strides=(16 * 384, 384, 2)), -2, "unit d-stride"),
    ("forced_misaligned", dict(variant=MFMA16DV, v_strides=(16 * 132, 132, 1)), -2, "16-byte aligned rows"),
    ("forced_misaligned_ptr", dict(variant=MFMA16DV, ptr=0x1008), -2, "16-byte aligned rows"),
    ("mfma16d_w4", dict(variant=9), -2, "variant 9"), ("a64", dict(variant=24), -2, "variant 24"), ("unknown", dict(variant=99), -2, "variant 99"),
    ("mfma16d_at_equal_d", dict(variant=8, d=128, d_v=128), -2, "variant 8"),
]
MATRIX, VALU = "mfma16dv kernel launch failed", "generic kernel launch failed"
VALID = [  # (name, arguments, the first launch)
    ("auto", dict(), MATRIX), ("auto_plain_entry", dict(plain=True), MATRIX), ("auto_f16", dict(dtype=F16), MATRIX),
    ("forced", dict(variant=MFMA16DV), MATRIX), ("auto_gqa", dict(H_kv=2), MATRIX), ("forced_mqa", dict(variant=MFMA16DV, H_kv=1), MATRIX),
    ("fused_buffer", dict(k_strides=(16 * 320, 320, 1), v_strides=(16 * 320, 320, 1)), MATRIX),
    ("generic", dict(variant=1), VALU), ("auto_f32", dict(dtype=F32), VALU), ("auto_f64", dict(dtype=F64), VALU),
    ("auto_128_64", dict(d=128, d_v=64), VALU), ("auto_40_72", dict(d=40, d_v=72), VALU), ("auto_512_512", dict(d=512, d_v=512), VALU),
    ("auto_dstride2", dict(k_strides=(16 * 384, 384, 2)), VALU), ("auto_misaligned", dict(v_strides=(16 * 132, 132, 1)), VALU),
    ("auto_1_1", dict(d=1, d_v=1), VALU),
    # d_v == d: AUTO is the varlen table, GENERIC the varlen kernel
    ("auto_128_128", dict(d=128, d_v=128), "mfma16d kernel launch failed"), ("generic_128_128", dict(d=128, d_v=128, variant=1), VALU),
]


def _child():
    if torch.cuda.device_count() != 0:
        return {"skipped": "a device is visible"}
    return {name: _call(**kw) for name, kw, *_ in ERRORS + VALID}


@pytest.fixture(scope="module")
def calls():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    run = subprocess.run([sys.executable, os.path.abspath(__file__), "--calls"], env=env, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    got = json.loads(run.stdout.strip().splitlines()[-1])
    if "skipped" in got:
        pytest.skip(got["skipped"])
    return got


@pytest.mark.parametrize("name,code,needle", [(n, c, s) for n, _, c, s in ERRORS])
def test_argument_errors_before_any_launch(calls, name, code, needle):
    rc, msg = calls[name]
    assert rc == code and needle in msg and "launch failed" not in msg, (rc, msg)


@pytest.mark.parametrize("name,first", [(n, f) for n, _, f in VALID])
def test_a_valid_call_fails_only_at_its_first_launch(calls, name, first):
    rc, msg = calls[name]
    assert rc == -4 and msg.endswith(first), (rc, msg)


def test_python_surface_errors():
    bf = torch.bfloat16
    Q, K, V = torch.zeros(7, 4, 192, dtype=bf), torch.zeros(9, 2, 192, dtype=bf), torch.zeros(9, 2, 128, dtype=bf)
    cu = torch.tensor([0, 2, 7], dtype=torch.int32)
    cuk = torch.tensor([0, 4, 9], dtype=torch.int32)

    def check(**kw):
        return T.check_varlen_dv_args(kw.pop("Q", Q), kw.pop("K", K), kw.pop("V", V), kw.pop("cu_q", cu), kw.pop("cu_k", cuk),
                                      kw.pop("max_q", 5), kw.pop("max_k", 5), kw.pop("window", None))

    check()
    check(V=torch.zeros(9, 2, 1, dtype=bf))
    check(V=torch.zeros(9, 2, 512, dtype=bf))
    check(V=K, window=(64, 0))                                         # d_v == d is a valid call
    check(K=torch.zeros(9, 2, 320, dtype=bf)[..., :192], V=torch.zeros(9, 2, 320, dtype=bf)[..., 192:])   # strided views
    for kw, needle in ((dict(V=torch.zeros(9, 2, 0, dtype=bf)), "d_v"), (dict(V=torch.zeros(9, 2, 513, dtype=bf)), "d_v"),
                       (dict(V=torch.zeros(8, 2, 128, dtype=bf)), "total_k"), (dict(V=torch.zeros(9, 4, 128, dtype=bf)), "H_kv"),
                       (dict(V=V[0]), "(total, H, d)"), (dict(V=V.half()), "same dtype"), (dict(Q=Q.half()), "same dtype"),
                       (dict(K=torch.zeros(9, 2, 128, dtype=bf)), "Q's H and d"), (dict(K=torch.zeros(9, 3, 192, dtype=bf), V=torch.zeros(9, 3, 128, dtype=bf)), "H_kv"),
                       (dict(cu_q=cu.long()), "cu_seqlens_q"), (dict(cu_k=cuk[:2]), "B + 1"), (dict(max_q=-1), "max_seqlen_q"),
                       (dict(max_k=2.0), "max_seqlen_k"), (dict(window=(-2, 0)), "window"),
                       (dict(Q=Q.to(torch.float8_e5m2), K=K.to(torch.float8_e5m2), V=V.to(torch.float8_e5m2)), "not supported")):
        with pytest.raises(ValueError, match=re.escape(needle)):
            check(**kw)
    # the surface: the device named must be the tensors', a variant one of this call's, and CPU tensors reach no kernel
    args = (Q, K, V, cu, cuk, 5, 5)
    with pytest.raises(ValueError, match="is not the device"):
        fa.flash_attention_mla_prefill_forward(*args, "cuda:0")
    with pytest.raises(NotImplementedError):
        fa.flash_attention_mla_prefill_forward(*args, "cpu")
    with pytest.raises(NotImplementedError):
        fa.flash_attention_mla_prefill_forward(*args, "cpu", causal=True, scale=0.07, window=(64, 0), variant="mfma16dv")


def test_the_other_wrappers_still_refuse_a_value_width_of_its_own():
    bf = torch.bfloat16
    Q, K, V = torch.zeros(7, 4, 192, dtype=bf), torch.zeros(7, 4, 192, dtype=bf), torch.zeros(7, 4, 128, dtype=bf)
    cu = torch.tensor([0, 2, 7], dtype=torch.int32)
    with pytest.raises(ValueError, match=re.escape("varlen: K and V must be (total_k, H, d) with Q's H and d")):
        T.check_varlen_args(Q, K, V, cu, cu, 5, 5, None)
    with pytest.raises(AssertionError):
        fa.flash_attention_forward(Q[None], K[None], V[None], "cpu")
    with pytest.raises(AssertionError):
        fa.flash_attention_backward(Q[None], K[None], V[None], Q[None], Q[None], Q[None, ..., :1], "cpu")


if __name__ == "__main__":
    if sys.argv[1:] != ["--calls"]:
        sys.exit(__doc__)
    print(json.dumps(_child()))
