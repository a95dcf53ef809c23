"""Every backward kernel (include/fa2_bwd.h: mfma16, mfma32, generic and the auto choice) element by element against
oracle/fa2_bwd_arith.py, the restatement of its own arithmetic, fed with the forward's real O and L.

The restatement runs in fp64 on the device; oracle.fa2_bwd_arith.compare is the one comparison (its bars: minimum fraction
of bit-identical elements, and every element within one output ulp + one rounding step of a P / dS term times the largest
operand + fp32-order terms; the model is written in the module's docstring, and tests/test_bwd_arith.py shows on the CPU
that errors planted in the arithmetic fail it).  Large problems are checked on sampled heads.
"""
import math

import pytest
import torch

import flash_attention_dlrs_amd as fa
from flash_attention_dlrs_amd import _lib
from flash_attention_dlrs_amd import flash_attention_torch as ft
from flash_attention_dlrs_amd.flash_attention_torch import forward_head_size, next_power_of_2
from oracle import fa2_bwd_arith as A

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NS = [1, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 2048]   # 32 / 64 / 128-row tile and owner-block edges
DISTS = ["normal", "spread", "jump", "onehot"]


def auto_kernel(dtype, d, scale):
    """the kernel fa2_bwd picks for contiguous, aligned tensors (fa2_bwd_api.hip run(), the *_supports functions)"""
    if d in (64, 128) and scale > 0:
        if dtype in (torch.float16, torch.bfloat16):
            return "mfma16"
        if dtype == torch.float32:
            return "mfma32"
    return "generic"


def draw(B, H, N, d, dtype, dist, seed):
    """Q, K, V, dO on the device.  normal: N(0, 1) (the benchmarked inputs: large |L|); spread: N(0, 1/4); jump: the last
    query's maximum sits on a key of the last key tile, far above the rest; onehot: every query has one key (its own
    position) far above the others; tiny_do: N(0, 1/4) with dO scaled by 2^-12 (f16: most dS terms subnormal)"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    sp = 1.0 if dist == "normal" else 0.5
    Q, K, V, dO = (torch.randn(B, H, N, d, generator=g, device=DEV) * sp for _ in range(4))
    if dist == "jump":
        K[:, :, max(0, N - 3)] = Q[:, :, N - 1] * 2.0
    elif dist == "onehot":
        K = K * 0.25 + Q * 3.0
    elif dist == "tiny_do":
        dO = dO * 2.0 ** -12
    return tuple(t.to(dtype) for t in (Q, K, V, dO))


def fwd(Q, K, V, causal, scale):
    O, L = fa.flash_attention_forward(Q, K, V, DEV, causal=causal, scale=scale)
    return O, L


class _Ctx:
    def save_for_backward(self, *t):
        self.saved_tensors = t


def autograd_forward(Q, K, V, causal, scale):
    """O and the saved L of FlashAttention's forward (the code path of .apply, with a stand-in for autograd's ctx)"""
    ctx = _Ctx()
    O = ft._forward_impl(ctx, Q.detach(), K.detach(), V.detach(), causal, scale)
    return O, ctx.saved_tensors[4]


def check(Q, K, V, O, L, dO, got, causal, scale, kernel, what, heads=None):
    """compare on all heads, or on the listed (b, h) pairs"""
    if heads is None:
        ref = A.restate(Q, K, V, O, L, dO, causal, scale, kernel)
        return A.assert_close(got, ref, (what, kernel))
    for b, h in heads:
        sl = lambda t: t[b:b + 1, h:h + 1]
        ref = A.restate(*(sl(t) for t in (Q, K, V, O, L, dO)), causal, scale, kernel)
        A.assert_close(tuple(sl(t) for t in got), ref, (what, kernel, b, h))


def run_case(dtype, d, N, causal, variant, scale, dist, B=1, H=2, seed=0):
    Q, K, V, dO = draw(B, H, N, d, dtype, dist, seed)
    O, L = fwd(Q, K, V, causal, scale)
    got = fa.flash_attention_backward(Q, K, V, O, dO, L, DEV, causal=causal, scale=scale, variant=variant)
    kernel = auto_kernel(dtype, d, scale) if variant == "auto" else variant
    check(Q, K, V, O, L, dO, got, causal, scale, kernel, (str(dtype), d, N, causal, variant, scale, dist))


def scale_of(k, d):
    return (1.0, 1 / math.sqrt(d), 0.3)[k % 3]


def _dist_scale(i, d):
    """(dist, scale) for the i-th N of a row of the matrix: N(0, 1) always at scale 1 (the benchmarked pairing), the others
    cycling through the three scales"""
    dist = DISTS[i % 4]
    return dist, (1.0 if dist == "normal" else scale_of(i // 4 + i, d))


# ----------------------------------------------------------------------------- the variant matrix
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_mfma16(dtype, d, causal):
    for i, N in enumerate(NS):
        dist, scale = _dist_scale(i, d)
        run_case(dtype, d, N, causal, "mfma16", scale, dist, seed=i)
    if dtype == torch.float16:     # dS below 2^-14: the f16 conversion's subnormal range
        run_case(dtype, d, 300, causal, "mfma16", 0.3, "tiny_do", seed=99)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d", [64, 128])
def test_mfma32(d, causal):
    for i, N in enumerate(NS):
        dist, scale = _dist_scale(i, d)
        run_case(torch.float32, d, N, causal, "mfma32", scale, dist, seed=i)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_generic(dtype, causal):
    for j, d in enumerate((16, 32, 64, 256)):
        for i, N in enumerate((1, 17, 65, 129, 257)):
            dist, scale = _dist_scale(i + j, d)
            run_case(dtype, d, N, causal, "generic", scale, dist, seed=10 * j + i)
    if dtype == torch.float16:
        run_case(dtype, 32, 200, causal, "generic", 0.3, "tiny_do", seed=98)


@pytest.mark.parametrize("causal", [False, True])
def test_auto(causal):
    for k, (dtype, d, N) in enumerate(((torch.bfloat16, 128, 1000), (torch.float16, 64, 257), (torch.float32, 128, 129),
                                       (torch.bfloat16, 32, 129), (torch.float32, 16, 65))):
        run_case(dtype, d, N, causal, "auto", scale_of(k, d), DISTS[k % 4], seed=k)


@pytest.mark.parametrize("scale", [0.0, -0.5])
def test_nonpositive_scale_goes_to_generic(scale):
    """mfma16 / mfma32 refuse scale <= 0 (fa2_bwd_mfma16_supports); auto takes generic there and is right"""
    Q, K, V, dO = draw(1, 2, 130, 128, torch.bfloat16, "spread", 7)
    O, L = fwd(Q, K, V, True, scale)
    with pytest.raises(TypeError):
        fa.flash_attention_backward(Q, K, V, O, dO, L, DEV, causal=True, scale=scale, variant="mfma16")
    got = fa.flash_attention_backward(Q, K, V, O, dO, L, DEV, causal=True, scale=scale)
    gen = fa.flash_attention_backward(Q, K, V, O, dO, L, DEV, causal=True, scale=scale, variant="generic")
    assert all(torch.equal(a, b) for a, b in zip(got, gen))
    check(Q, K, V, O, L, dO, got, True, scale, "generic", scale)


# ----------------------------------------------------------------------------- layouts
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_bnhd_views_through_autograd(dtype, causal):
    """FlashAttention.apply on (B, N, H, d) storage viewed as (B, H, N, d), d = 128: the backward runs mfma16 on the views
    (bit-equal to a forced mfma16 launch), the gradients come back with the inputs' strides, and match the restatement"""
    B, N, H, d = 2, 321, 3, 128
    g = torch.Generator(device=DEV).manual_seed(5)
    Qs, Ks, Vs, Gs = ((torch.randn(B, N, H, d, generator=g, device=DEV) * 0.5).to(dtype) for _ in range(4))
    for t in (Qs, Ks, Vs):
        t.requires_grad_(True)
    Q, K, V, dO = (t.transpose(1, 2) for t in (Qs, Ks, Vs, Gs))
    out = fa.FlashAttention.apply(Q, K, V, causal, 0.3)
    grads = torch.autograd.grad(out, (Qs, Ks, Vs), dO)
    for gr, t in zip(grads, (Qs, Ks, Vs)):
        assert gr.stride() == t.stride()
    got = tuple(gr.transpose(1, 2) for gr in grads)
    Qd, Kd, Vd = (t.detach() for t in (Q, K, V))
    O, L = autograd_forward(Qd, Kd, Vd, causal, 0.3)
    assert torch.equal(O, out.detach())
    forced = fa.flash_attention_backward(Qd, Kd, Vd, O, dO, L, DEV, causal=causal, scale=0.3, variant="mfma16")
    assert all(torch.equal(a, b) for a, b in zip(got, forced))
    check(Qd, Kd, Vd, O, L, dO, got, causal, 0.3, "mfma16", "bnhd")


@pytest.mark.parametrize("causal", [False, True])
def test_do_broadcast_and_strided(causal):
    """a dO with strides (0, 0, 0, 1) (w.expand: backward_native hands it to mfma16 as it is) and one with stride(-1) = 2"""
    B, H, N, d = 2, 2, 200, 128
    Q, K, V, _ = draw(B, H, N, d, torch.bfloat16, "spread", 11)
    O, L = fwd(Q, K, V, causal, 1.0)
    w = (torch.randn(d, device=DEV) * 0.5).to(torch.bfloat16)
    dO = w.expand(B, H, N, d)
    assert dO.stride() == (0, 0, 0, 1)
    got = fa.flash_attention_backward(Q, K, V, O, dO, L, DEV, causal=causal, variant="mfma16")
    dense = fa.flash_attention_backward(Q, K, V, O, dO.contiguous(), L, DEV, causal=causal, variant="mfma16")
    assert all(torch.equal(a, b) for a, b in zip(got, dense))
    check(Q, K, V, O, L, dO, got, causal, 1.0, "mfma16", "expand")
    wide = (torch.randn(B, H, N, 2 * d, device=DEV) * 0.5).to(torch.bfloat16)
    dO = wide[..., ::2]
    assert dO.stride(-1) == 2
    got = fa.flash_attention_backward(Q, K, V, O, dO, L, DEV, causal=causal)
    check(Q, K, V, O, L, dO, got, causal, 1.0, "mfma16", "stride2")


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtype,d,variant", [(torch.bfloat16, 128, "mfma16"), (torch.float16, 64, "mfma16"),
                                             (torch.float32, 128, "mfma32"), (torch.float32, 64, "mfma32"),
                                             (torch.bfloat16, 32, "generic"), (torch.float16, 256, "generic")])
def test_canary_arenas(dtype, d, variant, causal):
    """dQ, dK, dV as views into arenas N + 8 rows and d + 8 columns wide, launched through _lib.fa2_bwd: nothing outside
    the views is written, and the views hold the restatement's result"""
    for N in (65, 257):
        B, H = 1, 2
        Q, K, V, dO = draw(B, H, N, d, dtype, "spread", N)
        O, L = fwd(Q, K, V, causal, 0.3)
        canary = -1234.5
        arenas = [torch.full((B, H, N + 8, d + 8), canary, dtype=dtype, device=DEV) for _ in range(3)]
        views = [a[:, :, :N, :d] for a in arenas]
        D = torch.empty(2, B, H, N, 1, dtype=torch.float32, device=DEV)
        _lib.fa2_bwd(Q, K, V, O, dO, L, *views, D, fa.convert_triton_dtype(dtype), causal=causal, scale=0.3,
                     variant=_lib.BWD_VARIANTS[variant])
        torch.cuda.synchronize()
        for a in arenas:
            assert (a[:, :, N:] == canary).all() and (a[:, :, :, d:] == canary).all(), (variant, N)
        check(Q, K, V, O, L, dO, tuple(views), causal, 0.3, variant, ("arena", N))


def test_32bit_offset_guard():
    """fa2_bwd_mfma16_supports: (N + 64) * row stride * 2 < 2^31 for every swept tensor.  Q (swept by the dK / dV launch)
    as a narrow slice of a wide buffer: just under the limit mfma16 runs it and is right, at the limit auto routes it to
    generic (mfma16 refuses it) and is right.  (O and L come from a forward of the same values in a dense Q.)"""
    N, d = 64, 128
    K, V, dO = (t for t in draw(1, 1, N, d, torch.bfloat16, "spread", 3)[1:])
    q = draw(1, 1, N, d, torch.bfloat16, "spread", 4)[0]
    for stride, kernel in (((1 << 31) // (2 * (N + 64))) - 8, "mfma16"), ((1 << 31) // (2 * (N + 64)), "generic"):
        buf = torch.empty(N, stride, dtype=torch.bfloat16, device=DEV)
        Q = buf[:, :d].view(1, 1, N, d)
        Q.copy_(q)
        assert Q.stride(2) == stride and ((N + 64) * stride * 2 < 2 ** 31) == (kernel == "mfma16")
        for causal in (False, True):
            O, L = fwd(q, K, V, causal, 1.0)
            got = fa.flash_attention_backward(Q, K, V, O, dO, L, DEV, causal=causal)
            if kernel == "mfma16":
                forced = fa.flash_attention_backward(Q, K, V, O, dO, L, DEV, causal=causal, variant="mfma16")
                assert all(torch.equal(a, b) for a, b in zip(got, forced))
            else:
                with pytest.raises(TypeError):
                    fa.flash_attention_backward(Q, K, V, O, dO, L, DEV, causal=causal, variant="mfma16")
            check(Q, K, V, O, L, dO, got, causal, 1.0, kernel, ("guard", stride))
        del buf, Q
        torch.cuda.empty_cache()


# ----------------------------------------------------------------------------- full size
def test_c3_as_benchmarked():
    """bench.py's c3: B4 H32 N4096 d128 bf16, causal, scale 1, N(0, 1) drawn as bench.py draws it; heads (0, 0), (2, 16),
    (3, 31) restated in fp64.  Heads 0-7 run alone are bit-identical to the same heads of the full run."""
    torch.manual_seed(42)
    Q, K, V = (torch.randn(4, 32, 4096, 128, device=DEV).to(torch.bfloat16) for _ in range(3))
    O, L = fwd(Q, K, V, True, 1.0)
    dO = torch.randn_like(Q)
    got = fa.flash_attention_backward(Q, K, V, O, dO, L, DEV, causal=True)
    check(Q, K, V, O, L, dO, got, True, 1.0, "mfma16", "c3", heads=[(0, 0), (2, 16), (3, 31)])
    sl = lambda t: t[:, :8].contiguous()
    part = fa.flash_attention_backward(sl(Q), sl(K), sl(V), sl(O), sl(dO), sl(L), DEV, causal=True)
    for a, b in zip(part, got):
        assert torch.equal(a, b[:, :8])


def test_c2_shape():
    """BASELINE configs[1]: B2 H8 N1024 d64 f16 (non-causal, scale 1); four heads restated"""
    Q, K, V, dO = draw(2, 8, 1024, 64, torch.float16, "normal", 12)
    O, L = fwd(Q, K, V, False, 1.0)
    got = fa.flash_attention_backward(Q, K, V, O, dO, L, DEV)
    check(Q, K, V, O, L, dO, got, False, 1.0, "mfma16", "c2", heads=[(0, 0), (0, 5), (1, 3), (1, 7)])


# ----------------------------------------------------------------------------- the forward's head-size routing
@pytest.mark.parametrize("d,H", [(32, 64), (24, 64), (40, 64), (48, 64), (96, 32), (20, 64), (100, 64)])
def test_backward_through_forward_head_size(d, H):
    """FlashAttention.apply, bf16, causal, N = 4096: B H N = 256 Ki rows (96: 128 Ki), where forward_head_size pads
    d < 64 to 64 and 64 < d < 128 to 128.  The backward pads to the next power of two (d = 32: not at all, and O arrives
    as a view with row stride 64) and runs the kernel auto picks at that head size; two heads restated"""
    B, N = 1, 4096
    dtype = torch.bfloat16
    g = torch.Generator(device=DEV).manual_seed(d)
    Q, K, V, dO = ((torch.randn(B, H, N, d, generator=g, device=DEV) * 0.5).to(dtype) for _ in range(4))
    d_fwd, d_bwd = forward_head_size(dtype, B, H, N, d, True), max(next_power_of_2(d), 16)
    assert d_fwd in (64, 128) and d_fwd != d
    Qg, Kg, Vg = (t.clone().requires_grad_(True) for t in (Q, K, V))
    out = fa.FlashAttention.apply(Qg, Kg, Vg, True, 1.0)
    got = torch.autograd.grad(out, (Qg, Kg, Vg), dO)
    O, L = autograd_forward(Q, K, V, True, 1.0)
    assert torch.equal(O, out.detach())
    if d == 32:
        assert O.stride(2) == 64
    check(Q, K, V, O, L, dO, got, True, 1.0, auto_kernel(dtype, d_bwd, 1.0), ("head size", d, d_bwd),
          heads=[(0, 0), (0, H - 1)])
