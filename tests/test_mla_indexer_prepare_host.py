"""The indexer's front end (hadamard_rotate, mla_indexer_prepare_queries, the rotary / hadamard keywords of mla_indexer_append) without
a GPU: the torch restatement of the Hadamard transform against the matrix product in fp64, the wrappers' errors, and the four C entry
points' symbols, codes and messages (fake pointers, nothing is launched)."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import flash_attention_dlrs_amd as fa
from flash_attention_dlrs_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fa2_mla_indexer_prepare_q", "fa2_mla_indexer_prepare_q_varlen", "fa2_mla_indexer_append_rot", "fa2_mla_indexer_append_varlen_rot")
F16, BF16, F32, E4 = _lib.FA2_DTYPE_F16, _lib.FA2_DTYPE_BF16, _lib.FA2_DTYPE_F32, _lib.FA2_DTYPE_F8E4M3
i64 = lambda t: None if t is None else (ctypes.c_int64 * len(t))(*t)

H128 = torch.ones(1, 1, dtype=torch.float64)
for _ in range(7):
    H128 = torch.kron(torch.tensor([[1.0, 1.0], [1.0, -1.0]], dtype=torch.float64), H128)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_hadamard_rotate_against_the_fp64_matrix_product(dtype):
    """|h - H x / sqrt(128)| <= 7 * 2^-24 * ||x||_1 / sqrt(128) (seven fp32 stages, each adding at most a relative 2^-24 of partial
    sums that ||x||_1 bounds) + half an ulp of the 16-bit result, the ulp of h's own binade (the subnormal one below the format's
    smallest normal number)."""
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(64, 128, generator=g) * 2.0 ** torch.randint(-6, 7, (64, 1), generator=g)).to(dtype)
    ref = x.double() @ H128 / 128 ** 0.5
    h = fa.hadamard_rotate(x)
    mant, emin = (10, -14) if dtype == torch.float16 else (7, -126)
    half_ulp = torch.ldexp(torch.tensor(0.5, dtype=torch.float64), (torch.frexp(h.double())[1] - 1).clamp(min=emin) - mant)
    bound = 7 * 2.0 ** -24 * x.double().abs().sum(-1, keepdim=True) / 128 ** 0.5 + half_ulp
    err = (h.double() - ref).abs()
    assert (err <= bound).all(), (err / bound).max()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_hadamard_rotate_is_exact_on_small_integers(dtype):
    """Integers in [-3, 3]: every stage sum is an integer below 2^9, exact in fp32 in any order; what remains is one fp32 product with
    float32(128 ** -0.5) and one rounding to the dtype, both IEEE."""
    x = torch.randint(-3, 4, (32, 128), generator=torch.Generator().manual_seed(1))
    want = ((x.double() @ H128).float() * torch.tensor(128 ** -0.5, dtype=torch.float32)).to(dtype)
    assert torch.equal(fa.hadamard_rotate(x.to(dtype)), want)
    assert torch.equal(fa.hadamard_rotate(x.to(dtype).T.contiguous().T[:, :128]), want)  # a strided view


def test_wrapper_errors_name_their_argument():
    q, w, lens = torch.zeros(2, 4, 3, 128, dtype=torch.bfloat16), torch.zeros(2, 4, 3), torch.zeros(2, dtype=torch.int32)
    cos = torch.zeros(8, 32, dtype=torch.bfloat16)
    k_idx, k_new = torch.zeros(2, 16, 128, dtype=torch.bfloat16), torch.zeros(2, 3, 128, dtype=torch.bfloat16)
    cu = torch.tensor([0, 3, 6], dtype=torch.int32)
    prepare = lambda q=q, w=w, **kw: fa.mla_indexer_prepare_queries(q, w, lens, **kw)
    packed = lambda q=q, w=w, **kw: fa.mla_indexer_prepare_queries_varlen(q.flatten(0, 1)[:6], w.flatten(0, 1)[:6], cu, 3, lens, **kw)
    append = lambda k_idx=k_idx, k_new=k_new, **kw: fa.mla_indexer_append(k_idx, k_new, lens, **kw)
    for call, kw, needle in (
            (prepare, dict(q=q[..., :96]), "d_I = 128"), (prepare, dict(q=q.float()), "q_idx must be float16 or bfloat16"),
            (prepare, dict(q=torch.zeros(2, 4, 3, 256, dtype=torch.bfloat16)[..., ::2]), "q_idx needs a unit column stride"),
            (prepare, dict(rotary_cos=cos), "rotary_cos and rotary_sin go together"),
            (prepare, dict(rotary_cos=torch.zeros(8, 65, dtype=torch.bfloat16), rotary_sin=torch.zeros(8, 65, dtype=torch.bfloat16)), "rotary_dim = 130"),
            (prepare, dict(w=w[:, :2]), "weights must be a float32 tensor"), (prepare, dict(dtype=torch.float32), "dtype must be"),
            (prepare, dict(weight_scale=float("inf")), "weight_scale"), (packed, dict(q=q.float()), "q_idx must be float16 or bfloat16"),
            (append, dict(k_idx=k_idx[..., :96], k_new=k_new[..., :96], hadamard=True), "d_I = 128"),
            (append, dict(k_idx=k_idx.float(), k_new=k_new.float(), hadamard=True), "k_new must be float16 or bfloat16"),
            (append, dict(rotary_sin=cos), "rotary_cos and rotary_sin go together"),
            (append, dict(k_new=torch.zeros(2, 3, 256, dtype=torch.bfloat16)[..., ::2], rotary_cos=cos, rotary_sin=cos), "k_new needs a unit column stride")):
        with pytest.raises(ValueError, match=re.escape(needle)):
            call(**kw)


def test_symbols_declared_bound_listed_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fa2_fwd.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exports = open(os.path.join(ROOT, "flash_attention_dlrs_amd", "csrc", "fa2_exports.map")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS and re.search(rf"\b{name}\s*\(", header) and re.search(rf"\bT {name}\b", out), name
        assert re.search(rf"\b{name};", exports) and getattr(_lib.lib(), name).argtypes is not None, name


def _prepare(packed, q=0x1000, q_col=1, w=0x2000, q_out=0x3000, lens=0x5000, cos=0x6000, sin=0x7000, rd=64, S_rot=100, scale=1.0, B=3,
             d_I=128, dtype=BF16, out=E4):
    rot = (cos, sin, 32, 32, S_rot, rd, 0, 1)
    if packed:
        rc = _lib.lib().fa2_mla_indexer_prepare_q_varlen(q, i64((8 * 128, 128, q_col)), w, i64((8, 1)), q_out, 0x4000, 0x8000, lens, *rot, scale,
                                                         B, 8, 9, 4, d_I, dtype, out, None)
    else:
        rc = _lib.lib().fa2_mla_indexer_prepare_q(q, i64((1024, 128, 128, q_col)), w, i64((8, 1, 1)), q_out, 0x4000, lens, *rot, scale,
                                                  B, 8, 1, d_I, dtype, out, None)
    return rc, _lib.lib().fa2_last_error().decode()


def _append(packed, k_idx=0x1000, k_new=0x3000, k_col=1, cos=0x6000, sin=0x7000, rd=64, had=1, d_I=128, dtype=BF16, k_dtype=E4):
    head = (k_idx, i64((192 * d_I, d_I, 1)), 0x2000 if k_dtype == E4 else None, i64((192, 1)), None, 0, k_new)
    rot = (cos, sin, 32, 32, 100, rd, 0, had)
    if packed:
        rc = _lib.lib().fa2_mla_indexer_append_varlen_rot(*head, i64((d_I, k_col)), 0x8000, 0x4000, 0x5000, *rot, 3, 9, 4, 192, 0, 0, 0, d_I,
                                                          dtype, k_dtype, None)
    else:
        rc = _lib.lib().fa2_mla_indexer_append_rot(*head, i64((d_I, d_I, k_col)), 0x4000, 0x5000, *rot, 3, 1, 192, 0, 0, 0, d_I, dtype, k_dtype, None)
    return rc, _lib.lib().fa2_last_error().decode()


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("call,kwargs,code,needle", [
    (_prepare, dict(q=None), -1, "null q_idx"), (_prepare, dict(q_out=None), -1, "null q_out"), (_prepare, dict(w=None), -1, "null weights"),
    (_prepare, dict(q_col=2), -1, "q_idx needs a unit column stride"), (_prepare, dict(d_I=64), -2, "d_I=64"),
    (_prepare, dict(dtype=F32), -2, "(q_idx) must be FA2_DTYPE_F16 or FA2_DTYPE_BF16"), (_prepare, dict(out=F32), -2, "out_dtype_enum"),
    (_prepare, dict(sin=None), -1, "null rotary_sin"), (_prepare, dict(rd=63), -1, "rotary_dim even in [2, 128]"),
    (_prepare, dict(rd=130), -1, "rotary_dim even in [2, 128]"), (_prepare, dict(S_rot=0), -1, "S_rot must be >= 1"),
    (_prepare, dict(lens=None), -1, "null cache_seqlens with rotary tables"), (_prepare, dict(scale=float("nan")), -1, "weight_scale must be finite"),
    (_prepare, dict(B=0), -1, "B must be in [1, 65535]"), (_prepare, dict(q_out=0x3008), -1, "q_out must be 16-byte aligned"),
    (_append, dict(k_idx=None), -1, "null k_idx"), (_append, dict(cos=None), -1, "null rotary_cos"), (_append, dict(rd=66, d_I=64), -2, "d_I=64"),
    (_append, dict(rd=7), -1, "rotary_dim even in [2, 128]"), (_append, dict(k_col=2), -1, "k_new needs a unit column stride"),
    (_append, dict(dtype=F32, k_dtype=F32), -2, "(k_new) must be FA2_DTYPE_F16 or FA2_DTYPE_BF16"),
    (_append, dict(cos=None, sin=None, d_I=96), -2, "d_I=96"),                        # hadamard alone asks for 128 columns too
])
def test_argument_errors_before_any_launch(call, kwargs, code, needle, packed):
    rc, msg = call(packed, **kwargs)
    assert rc == code and needle in msg, (rc, msg)
