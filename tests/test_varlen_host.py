"""Variable-length (packed) attention without a GPU: the C-ABI argument checks (returned before any launch), the exported symbols,
the Python validation, varlen_mask against its definition and the fp64 reference against an independent dense formulation."""
import ctypes
import math
import subprocess

import pytest
import torch

from flash_attention_dlrs_amd import _lib, varlen_mask
from flash_attention_dlrs_amd.flash_attention_torch import check_varlen_args

VARLEN_SYMBOLS = ("fa2_fwd_varlen", "fa2_fwd_varlen_variant", "fa2_bwd_varlen", "fa2_bwd_varlen_variant")


def varlen_reference(Q, K, V, cu_q, cu_k, causal=False, scale=1.0, window=None):
    """fp64 truth of a packed batch: one sequence at a time, bottom-right aligned mask.  Returns O (total_q, H, d) and the
    log2-domain L (H, total_q); rows without a visible key get O = 0 and L = +inf."""
    q, k, v = (t.double() for t in (Q, K, V))
    O = torch.zeros(q.shape, dtype=torch.float64)
    L = torch.full((q.shape[1], q.shape[0]), math.inf, dtype=torch.float64)
    cq, ck = cu_q.tolist(), cu_k.tolist()
    left, right = (-1, -1) if window is None else window
    if causal:
        right = 0
    for b in range(len(cq) - 1):
        q0, q1, k0, k1 = cq[b], cq[b + 1], ck[b], ck[b + 1]
        nq, nk = q1 - q0, k1 - k0
        if nq == 0:
            continue
        for i in range(nq):
            c = i + nk - nq
            lo = 0 if left < 0 else max(c - left, 0)
            hi = nk - 1 if right < 0 else min(c + right, nk - 1)
            if nk == 0 or hi < lo:
                continue
            s = torch.einsum("hd,khd->hk", q[q0 + i], k[k0 + lo:k0 + hi + 1]) * scale
            p = torch.softmax(s, -1)
            O[q0 + i] = torch.einsum("hk,khd->hd", p, v[k0 + lo:k0 + hi + 1])
            L[:, q0 + i] = torch.logsumexp(s, -1) * math.log2(math.e)
    return O, L


def _cu(lengths):
    return torch.tensor([0] + list(torch.tensor(lengths).cumsum(0).tolist()), dtype=torch.int32)


@pytest.mark.parametrize("causal,window", [(False, None), (True, None), (False, (5, 3)), (True, (7, -1)), (False, (-1, 0))])
def test_varlen_reference_matches_dense_block_diagonal(causal, window):
    g = torch.Generator().manual_seed(3)
    lq, lk = [5, 0, 17, 9, 3, 12], [8, 4, 17, 2, 0, 20]  # N_q < N_k, N_q > N_k, empty on either side
    cu_q, cu_k = _cu(lq), _cu(lk)
    H, d = 2, 8
    Q, K, V = (torch.randn(sum(n), H, d, generator=g, dtype=torch.float64) for n in (lq, lk, lk))
    O, L = varlen_reference(Q, K, V, cu_q, cu_k, causal, 0.6, window)
    # independent: one dense (total_q, total_k) problem per head with the block-diagonal, bottom-right mask built by hand
    mask = torch.zeros(sum(lq), sum(lk), dtype=torch.bool)
    for b in range(len(lq)):
        for i in range(lq[b]):
            for j in range(lk[b]):
                c = i + lk[b] - lq[b]
                ok = (j <= c) if causal else True
                if window is not None:
                    ok = ok and (window[0] < 0 or j >= c - window[0]) and (causal or window[1] < 0 or j <= c + window[1])
                mask[cu_q[b] + i, cu_k[b] + j] = ok
    S = torch.einsum("qhd,khd->hqk", Q, K) * 0.6
    S = S.masked_fill(~mask, -math.inf)
    rows = mask.any(-1)
    P = torch.softmax(S[:, rows], -1)
    O_ref = torch.zeros_like(O)
    O_ref[rows] = torch.einsum("hqk,khd->qhd", P, V)
    L_ref = torch.full_like(L, math.inf)
    L_ref[:, rows] = torch.logsumexp(S[:, rows], -1) * math.log2(math.e)
    assert torch.allclose(O, O_ref, atol=1e-12)
    assert torch.equal(torch.isinf(L), torch.isinf(L_ref)) and torch.allclose(L[:, rows], L_ref[:, rows], atol=1e-12)


@pytest.mark.parametrize("causal,window", [(False, None), (True, None), (False, (2, 1)), (True, (3, 5)), (False, (-1, 0)),
                                           (False, (0, -1))])
def test_varlen_mask_matches_definition(causal, window):
    lq, lk = [4, 6, 0, 3, 5], [4, 2, 3, 0, 9]  # equal, N_q > N_k (causal empty rows), empty sequences
    cu_q, cu_k = _cu(lq), _cu(lk)
    m = varlen_mask(cu_q, cu_k, causal, window)
    assert m.shape == (sum(lq), sum(lk))
    left, right = (-1, -1) if window is None else window
    if causal:
        right = 0
    for b in range(len(lq)):
        for qt in range(sum(lq)):
            for kt in range(sum(lk)):
                inside = cu_q[b] <= qt < cu_q[b + 1] and cu_k[b] <= kt < cu_k[b + 1]
                if not inside:
                    if cu_q[b] <= qt < cu_q[b + 1]:
                        assert not m[qt, kt]
                    continue
                i, j = qt - int(cu_q[b]), kt - int(cu_k[b])
                c = i + lk[b] - lq[b]
                want = (left < 0 or j >= c - left) and (right < 0 or j <= c + right)
                assert bool(m[qt, kt]) == want, (b, i, j)
    # causal with N_q > N_k: the first N_q - N_k query rows of sequence 1 see nothing
    if causal and window is None:
        assert not m[4:8].any() and m[8:10].any()


def test_varlen_mask_equal_lengths_is_the_dense_mask():
    cu = _cu([7, 7])
    m = varlen_mask(cu, cu, True)
    tri = torch.ones(7, 7, dtype=torch.bool).tril()
    assert torch.equal(m[:7, :7], tri) and torch.equal(m[7:, 7:], tri) and not m[:7, 7:].any() and not m[7:, :7].any()


def _cpu_tensors(dtype=torch.float16, shape_q=(10, 2, 64), shape_k=(12, 2, 64)):
    return torch.zeros(shape_q, dtype=dtype), torch.zeros(shape_k, dtype=dtype), torch.zeros(shape_k, dtype=dtype)


def test_python_entry_points_require_a_cuda_device():
    from flash_attention_dlrs_amd.flash_attention_torch import varlen_forward
    Q, K, V = _cpu_tensors()
    with pytest.raises(NotImplementedError):
        varlen_forward(Q, K, V, _cu([10]), _cu([12]), 10, 12)


@pytest.mark.parametrize("case,msg", [
    ("fp8", "not supported"),
    ("shape", "(total, H, d)"),
    ("kv", "K and V"),
    ("dtype_mix", "same dtype"),
    ("cu_dtype", "int32"),
    ("cu_len", "B + 1"),
    ("cu_mismatch", "both have B + 1"),
    ("cu_strided", "contiguous"),
    ("max_neg", "max_seqlen_q"),
    ("window", "window"),
])
def test_python_validation_errors(case, msg):
    Q, K, V = _cpu_tensors()
    cu_q, cu_k, mq, mk, window = _cu([10]), _cu([12]), 10, 12, None
    if case == "fp8":
        Q, K, V = (t.to(torch.float8_e4m3fn) for t in (Q, K, V))
    elif case == "shape":
        Q = Q.unsqueeze(0)
    elif case == "kv":
        V = V[:5]
    elif case == "dtype_mix":
        K = K.float()
    elif case == "cu_dtype":
        cu_q = cu_q.long()
    elif case == "cu_len":
        cu_q, cu_k = cu_q[:1], cu_k[:1]
    elif case == "cu_mismatch":
        cu_k = _cu([6, 6])
    elif case == "cu_strided":
        cu_q = torch.arange(4, dtype=torch.int32)[::2]
    elif case == "max_neg":
        mq = -1
    elif case == "window":
        window = (-2, 0)
    with pytest.raises(ValueError, match=msg.replace("(", r"\(").replace(")", r"\)").replace("+", r"\+")):
        check_varlen_args(Q, K, V, cu_q, cu_k, mq, mk, window)
    check_varlen_args(*_cpu_tensors(), _cu([10]), _cu([12]), 10, 12, (3, -1))  # (and the good call passes)


def _i64(v):
    return (ctypes.c_int64 * len(v))(*v)


def _fwd(ptr=0x1000, cu=0x2000, B=2, H=2, d=64, mq=8, mk=8, tq=16, tk=16, wl=-1, wr=-1, dtype=None, variant=0):
    s = _i64((H * d, d, 1))
    return _lib.lib().fa2_fwd_varlen_variant(ptr, ptr, ptr, ptr, ptr, s, s, s, s, tq, cu, cu, B, H, d, mq, mk, tq, tk,
                                             _lib.FA2_DTYPE_BF16 if dtype is None else dtype, 0, 1.0, wl, wr, None, variant)


def _bwd(ptr=0x1000, cu=0x2000, B=2, H=2, d=64, mq=8, mk=8, tq=16, tk=16, wl=-1, wr=-1, dtype=None, variant=0):
    s = [_i64((H * d, d, 1)) for _ in range(8)]
    return _lib.lib().fa2_bwd_varlen_variant(ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, *s, tq, cu, cu, B, H, d, mq, mk,
                                             tq, tk, _lib.FA2_DTYPE_BF16 if dtype is None else dtype, 0, 1.0, wl, wr, None,
                                             variant)


@pytest.mark.parametrize("kw,word", [
    (dict(ptr=0), "null"), (dict(cu=0), "cu_seqlens_q"), (dict(B=0), "B"), (dict(B=-3), "B"),
    (dict(mq=-1), "max_seqlen"), (dict(mk=-5), "max_seqlen"), (dict(tq=-1), "total"), (dict(tk=-2), "total"),
    (dict(wl=-2), "window"), (dict(wr=-9), "window"),
])
def test_abi_rejects_bad_arguments_before_any_launch(kw, word):
    # every pointer here is a fake address: a launch would fault, so FA2_ERR_BAD_ARG proves the check came first
    for call in (_fwd, _bwd):
        assert call(**kw) == -1, (call.__name__, kw)
        assert word in _lib.lib().fa2_last_error().decode(), (call.__name__, kw, _lib.lib().fa2_last_error())


def test_abi_rejects_fp8_and_variants_without_a_varlen_form():
    for dt in (_lib.FA2_DTYPE_F8E4M3, _lib.FA2_DTYPE_F8E5M2):
        assert _fwd(dtype=dt) == -2 and "fp8" in _lib.lib().fa2_last_error().decode()
        assert _bwd(dtype=dt) == -2
    for v in (_lib.VARIANT_A64, _lib.VARIANTS["mfma16"], _lib.VARIANTS["mfma16h"], _lib.VARIANTS["mfma32"]):
        assert _fwd(variant=v) == -2 and "varlen" in _lib.lib().fa2_last_error().decode()
    assert _bwd(variant=_lib.BWD_VARIANTS["mfma32"]) == -2 and "varlen" in _lib.lib().fa2_last_error().decode()


def test_varlen_symbols_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    for name in VARLEN_SYMBOLS:
        assert f" T {name}\n" in out, name
        assert name in _lib.SYMBOLS + _lib.BWD_SYMBOLS
