"""The packed backward with a value head size of its own (fa2_bwd_varlen_dv, fa2_bwd_varlen_dv_variant), the part that needs no GPU:
the two exported symbols and the variant table, every argument error before any launch and which kernel a valid call launches
first (fake pointers, in a child process that sees no device), and the Python surface's errors on CPU tensors.

    python tests/test_mla_prefill_bwd_host.py --calls     the child: one JSON line, {"skipped": ...} or {name: [code, message]}"""
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

NEW = ("fa2_bwd_varlen_dv", "fa2_bwd_varlen_dv_variant")
MFMA16DV = 4
F32, F16, BF16, F8E5, F8E4, F64 = range(6)
TENSORS = ("Q", "K", "V", "O", "dO", "L", "dQ", "dK", "dV", "D")


def test_symbols_declared_bound_exported_and_listed():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fa2_bwd.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exports = open(os.path.join(ROOT, "flash_attention_dlrs_amd", "csrc", "fa2_exports.map")).read()
    for name in NEW:
        assert name in _lib.BWD_SYMBOLS
        assert re.search(rf"\b{name}\s*\(", header), name
        assert re.search(rf"\bT {name}\b", out), name
        assert re.search(rf"\b{name};", exports), name
        assert getattr(_lib.lib(), name).argtypes is not None
    assert re.search(r"#define\s+FA2_BWD_VARIANT_MFMA16DV\s+4\b", header)
    for name in ("flash_attention_mla_prefill_backward", "FlashAttentionMLAPrefill"):
        assert name in fa.__all__ and callable(getattr(fa, name))
    assert callable(_lib.fa2_bwd_varlen_dv) and callable(T.mla_prefill_backward)
    assert "Forward only" not in fa.flash_attention_mla_prefill_forward.__doc__


def test_variant_tables():
    assert _lib.BWD_VARLEN_DV_VARIANTS == {"auto": 0, "generic": 1, "mfma16dv": MFMA16DV}
    assert _lib.BWD_VARIANTS == {"auto": 0, "generic": 1, "mfma16": 2, "mfma32": 3}
    assert MFMA16DV not in _lib.BWD_VARIANTS.values()
    assert _lib.VARLEN_DV_VARIANTS == {"auto": 0, "generic": 1, "mfma16dv": 28}
    assert _lib.KVCACHE_VARIANTS == {"auto": 0, "generic": 1, "mfma16": 2}
    assert _lib.KVCACHE_MLA_VARIANTS == {"auto": 0, "generic": 1, "mla16": 3}


def _call(ptr=0x1000, nulls=(), cu=0x3000, B=3, H=16, H_kv=16, d=192, d_v=128, total=700, max_len=300, dtype=BF16, variant=0, scale=0.07,
          window=(-1, -1), plain=False, **strides):
    """a contiguous packed call on fake pointers -> (code, message; a launch failure's ends at "launch failed").  strides: q, k, v,
    o, do, dq, dk, dv = a 3-element override."""
    i64 = lambda v: (ctypes.c_int64 * len(v))(*v)
    t = [None if n in nulls else ptr for n in TENSORS]
    w = d_v if d_v > 0 else 128  # (a d_v that is refused still comes with usable strides)
    dflt = {"q": (H * d, d, 1), "k": (H_kv * d, d, 1), "v": (H_kv * w, w, 1), "o": (H * w, w, 1), "do": (H * w, w, 1),
            "dq": (H * d, d, 1), "dk": (H_kv * d, d, 1), "dv": (H_kv * w, w, 1)}
    assert set(strides) <= set(dflt)
    st = [i64(strides.get(n, dflt[n])) for n in ("q", "k", "v", "o", "do", "dq", "dk", "dv")]
    args = t + st + [total, cu, cu, B, H, H_kv, d, d_v, max_len, max_len, total, total, dtype, 1, scale, window[0], window[1], None]
    lib = _lib.lib()
    rc = lib.fa2_bwd_varlen_dv(*args) if plain else lib.fa2_bwd_varlen_dv_variant(*args, variant)
    msg = lib.fa2_last_error().decode()
    cut = msg.find("launch failed")
    return [rc, msg if cut < 0 else msg[:cut + len("launch failed")]]


FUSED = dict(k=(16 * 320, 320, 1), v=(16 * 320, 320, 1))
FUSED_OUT = dict(dk=(16 * 320, 320, 1), dv=(16 * 320, 320, 1))
ERRORS = [  # (name, arguments, code, what the message must hold)
    ("d_v_0", dict(d_v=0), -1, "d_v=0 must be in [1, 512]"), ("d_v_513", dict(d_v=513), -1, "d_v=513 must be in [1, 512]"),
    ("d_v_neg", dict(d_v=-128), -1, "d_v=-128 must be in [1, 512]"),
    ("d_513", dict(d=513), -2, "d=513 must be in [1, 512]"), ("d_0", dict(d=0), -1, "d=0"),       # the forward call's rule and codes
    ("gqa", dict(H=16, H_kv=3), -1, "H_kv must divide H"), ("h_kv_0", dict(H_kv=0), -1, "H_kv"),
    ("neg_stride", dict(v=(2048, -128, 1)), -1, "negative strides"),
    ("zero_stride_dK", dict(dk=(0, 192, 1)), -1, "must not alias themselves"),
    ("null_cu", dict(cu=None), -1, "null cu_seqlens_q"),
    ("fp8_e4m3", dict(dtype=F8E4), -2, "not supported"), ("fp8_e5m2", dict(dtype=F8E5), -2, "not supported"),
    ("B_0", dict(B=0), -1, "B (number of sequences)"), ("window", dict(window=(-2, 0)), -1, "window"),
    ("scale_nan", dict(scale=float("nan")), -1, "NaN"),
    # the order is fa2_bwd_varlen_gqa's, d_v last
    ("gqa_before_d_v", dict(H_kv=3, d_v=0), -1, "H_kv"), ("fp8_before_d_v", dict(dtype=F8E4, d_v=0), -2, "not supported"),
    ("stride_before_d_v", dict(q=(-1, 192, 1), d_v=0), -1, "negative strides"), ("nan_before_d_v", dict(scale=float("nan"), d_v=0), -1, "NaN"),
    ("d_before_d_v", dict(d=513, d_v=0), -2, "d=513"), ("null_before_d_v", dict(nulls=("D",), d_v=0), -1, "null D"),
    # a forced matrix kernel on what it cannot take, and what is no variant of this call
    ("forced_128_128", dict(variant=MFMA16DV, d=128, d_v=128), -2, "variant 4"),
    ("forced_192_192", dict(variant=MFMA16DV, d=192, d_v=192), -2, "variant 4"),
    ("forced_f32", dict(variant=MFMA16DV, dtype=F32), -2, "f16/bf16"),
    ("forced_dstride2", dict(variant=MFMA16DV, k=(16 * 384, 384, 2)), -2, "unit d-stride"),
    ("forced_misaligned", dict(variant=MFMA16DV, v=(16 * 132, 132, 1)), -2, "16-byte aligned rows"),
    ("forced_misaligned_out", dict(variant=MFMA16DV, dv=(16 * 132, 132, 1)), -2, "16-byte aligned rows"),
    ("forced_misaligned_ptr", dict(variant=MFMA16DV, ptr=0x1008), -2, "16-byte aligned rows"),
    ("mfma16_at_other_d_v", dict(variant=2), -2, "variant 2"), ("mfma32", dict(variant=3), -2, "variant 3"),
    ("unknown", dict(variant=99), -2, "variant 99"), ("mfma32_at_equal_d", dict(variant=3, d=128, d_v=128), -2, "variant 3"),
]
ERRORS += [("null_" + n, dict(nulls=(n,)), -1, "varlen backward: null " + n) for n in TENSORS]
MATRIX, VALU, MFMA16 = "backward mfma16dv launch failed", "generic backward launch failed", "backward mfma16 launch failed"
VALID = [  # (name, arguments, the first launch)
    ("auto", dict(), MATRIX), ("auto_plain_entry", dict(plain=True), MATRIX), ("auto_f16", dict(dtype=F16), MATRIX),
    ("forced", dict(variant=MFMA16DV), MATRIX), ("auto_gqa", dict(H_kv=2), MATRIX), ("forced_mqa", dict(variant=MFMA16DV, H_kv=1), MATRIX),
    ("fused_inputs", dict(**FUSED), MATRIX), ("fused_outputs", dict(**FUSED_OUT), MATRIX), ("fused_both", dict(**FUSED, **FUSED_OUT), MATRIX),
    ("generic", dict(variant=1), VALU), ("auto_f32", dict(dtype=F32), VALU), ("auto_f64", dict(dtype=F64), VALU),
    ("auto_128_64", dict(d=128, d_v=64), VALU), ("auto_40_72", dict(d=40, d_v=72), VALU), ("auto_1_1", dict(d=1, d_v=1, variant=1), VALU),
    ("auto_1_2", dict(d=1, d_v=2), VALU), ("auto_512_511", dict(d=512, d_v=511), VALU),
    ("auto_dstride2", dict(k=(16 * 384, 384, 2)), VALU), ("auto_misaligned", dict(v=(16 * 132, 132, 1)), VALU),
    # d_v == d: the varlen GQA call itself, through its table
    ("auto_128_128", dict(d=128, d_v=128), MFMA16), ("mfma16_128_128", dict(d=128, d_v=128, variant=2), MFMA16),
    ("generic_128_128", dict(d=128, d_v=128, variant=1), VALU), ("auto_40_40", dict(d=40, d_v=40), VALU),
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
    O, L = torch.zeros(7, 4, 128, dtype=bf), torch.zeros(4, 7, dtype=bf)
    cu = torch.tensor([0, 2, 7], dtype=torch.int32)
    cuk = torch.tensor([0, 4, 9], dtype=torch.int32)

    def run(**kw):
        variant = kw.pop("variant", "auto")
        args = [kw.pop(n, t) for n, t in (("Q", Q), ("K", K), ("V", V), ("O", O), ("dO", O), ("L", L), ("cu_q", cu), ("cu_k", cuk))]
        return T.mla_prefill_backward(*args, kw.pop("max_q", 5), kw.pop("max_k", 5), variant=variant, **kw)

    for kw, needle in ((dict(O=torch.zeros(7, 4, 192, dtype=bf)), "O and dO must be (7, 4, 128)"), (dict(dO=O.half()), "O and dO must be"),
                       (dict(dO=torch.zeros(7, 2, 128, dtype=bf)), "O and dO must be"), (dict(O=O.float()), "O and dO must be"),
                       (dict(L=torch.zeros(7, 4, dtype=bf)), "L must be (4, 7)"), (dict(L=torch.zeros(7, 4, dtype=bf).t()), "unit token stride"),
                       (dict(L=L.float()), "L must be"), (dict(variant="mfma16"), "variant must be one of"),
                       (dict(variant="mfma32"), "variant must be one of"), (dict(V=torch.zeros(9, 2, 513, dtype=bf)), "d_v"),
                       (dict(V=torch.zeros(9, 4, 128, dtype=bf)), "H_kv"), (dict(window=(-2, 0)), "window"), (dict(max_q=-1), "max_seqlen_q")):
        with pytest.raises(ValueError, match=re.escape(needle)):
            run(**kw)
    with pytest.raises(NotImplementedError):         # every rule met: CPU tensors still reach no kernel
        run()
    args = (Q, K, V, O, O, L, cu, cuk, 5, 5)
    with pytest.raises(ValueError, match="is not the device"):
        fa.flash_attention_mla_prefill_backward(*args, "cuda:0")
    with pytest.raises(NotImplementedError):
        fa.flash_attention_mla_prefill_backward(*args, "cpu", causal=True, scale=0.07, window=(64, 0), variant="mfma16dv")


def test_the_other_wrappers_still_refuse_a_value_width_of_its_own():
    bf = torch.bfloat16
    Q, K, V = torch.zeros(7, 4, 192, dtype=bf), torch.zeros(7, 4, 192, dtype=bf), torch.zeros(7, 4, 128, dtype=bf)
    cu = torch.tensor([0, 2, 7], dtype=torch.int32)
    with pytest.raises(ValueError, match=re.escape("varlen: K and V must be (total_k, H, d) with Q's H and d")):
        T.check_varlen_args(Q, K, V, cu, cu, 5, 5, None)
    with pytest.raises(AssertionError):
        fa.flash_attention_backward(Q[None], K[None], V[None], Q[None], Q[None], Q[None, ..., :1], "cpu")


if __name__ == "__main__":
    if sys.argv[1:] != ["--calls"]:
        sys.exit(__doc__)
    print(json.dumps(_child()))
