"""The KV-cache append on the GPU (fa2_kvcache_append, fa2_fwd_kvcache_append).  The yardstick throughout is BIT-EQUALITY with a
restatement computed on the CPU (tests/decode_append_restatement.py) and copied over: the whole cache after the call, viewed as
integers, equals a clone of the initial cache with the stored rows written in -- which also proves that no other byte changed --
and O, L of the fused call equal the existing call's on that expected cache, with the restated lengths and apply_rotary(Q).

The initial cache holds ordinary data in the rows below the lengths and a seeded random bit pattern, NaN encodings included, in
the rows past them; pools hold spare pages under a seeded permutation and table entries of pages the append does not touch are
-1 / 2^31 - 1."""
import math

import pytest
import torch

import flash_attention_dlrs_amd as fa
from flash_attention_dlrs_amd import _lib
from flash_attention_dlrs_amd.flash_attention_torch import convert_triton_dtype
from decode_append_restatement import INT_VIEW, bits, expected_append

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF, F16, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64
E4, E5 = torch.float8_e4m3fn, torch.float8_e5m2
INT_MAX = 2 ** 31 - 1
CAP = 256
SPARE = 3  # pool pages no table names
S_ROT = CAP + 8


def length_sets(P):
    """Four lengths a batch, out of [0, 1, 15, 16, 62, 63, 64, 127, cap - 3, cap - 1, cap]: with N_new = 3, P - 1 straddles a page
    boundary (15 and 63; 62 and 127 do as well), cap - 1 is partly dropped and cap wholly."""
    return [[0, 63, CAP - 1, CAP], [1, 15, 62, 127], [16, 64, CAP - 3, CAP - 1]]


def random_bits(shape, dtype, g):
    """A seeded random bit pattern in `dtype` (NaN and inf encodings included), on the CPU."""
    it = INT_VIEW[torch.empty(0, dtype=dtype).element_size()]
    info = torch.iinfo(it)
    return torch.randint(info.min, info.max, shape, generator=g, dtype=torch.int64).to(it).view(dtype)


class Problem:
    """One append problem on the CPU: Q, the new tokens, the initial cache (or pool and table), descales, rotary tables."""

    def __init__(self, dtype, kv, descales, d, P, H, H_kv, N_new, N_q, rd, interleaved, lens, seed, steps=1):
        g = torch.Generator().manual_seed(seed)
        B = len(lens)
        self.dtype, self.kv, self.P, self.lens, self.interleaved = dtype, kv, P, torch.tensor(lens, dtype=torch.int32), interleaved
        self.Q = (torch.randn(B, H, N_q, d, generator=g) * 0.5).to(dtype)
        self.k_new = (torch.randn(B, H_kv, N_new, d, generator=g) * 0.5).to(dtype)
        self.v_new = (torch.randn(B, H_kv, N_new, d, generator=g) * 0.5).to(dtype)
        K = (torch.randn(B, H_kv, CAP, d, generator=g) * 0.5).to(dtype)
        V = (torch.randn(B, H_kv, CAP, d, generator=g) * 0.5).to(dtype)
        self.kd = self.vd = None
        if kv is not None and descales:  # descales from quantize_kv_cache on the initial contents
            K, self.kd = fa.quantize_kv_cache(K, kv)
            V, self.vd = fa.quantize_kv_cache(V, kv)
        elif kv is not None:  # null descales: the cache holds the values themselves
            K, V = K.to(kv), V.to(kv)
        for t in (K, V):  # rows past the lengths: anything
            junk = random_bits(t.shape, t.dtype, g)
            for b, n in enumerate(lens):
                bits(t)[b, :, max(n, 0):] = bits(junk)[b, :, max(n, 0):]
        self.cos = self.sin = None
        if rd:
            ang = torch.rand(S_ROT, rd // 2, generator=g, dtype=torch.float64) * 6.283
            self.cos, self.sin = ang.cos().to(dtype), ang.sin().to(dtype)
        self.table = None
        if P is not None:  # scatter into a pool of B * max_blocks + SPARE pages under a seeded permutation
            mb = CAP // P
            nb = B * mb + SPARE
            perm = torch.randperm(nb, generator=g).to(torch.int32)
            self.table = perm[:B * mb].view(B, mb).clone()
            pools = []
            for t in (K, V):
                pool = random_bits((nb, H_kv, P, d), t.dtype, g)
                bits(pool)[self.table.view(-1).long()] = bits(t).view(B, H_kv, mb, P, d).permute(0, 2, 1, 3, 4).reshape(B * mb, H_kv, P, d)
                pools.append(pool)
            K, V = pools
            for b, n in enumerate(lens):  # entries of pages neither the old keys nor the append touch
                used = -(-min(max(n, 0) + steps * N_new, CAP) // P)
                for i in range(used, mb):
                    self.table[b, i] = (-1, INT_MAX)[(i - used) % 2]
        self.K, self.V = K, V

    def expected(self, K=None, V=None, lens=None, k_new=None, v_new=None):
        return expected_append(self.K if K is None else K, self.V if V is None else V, self.k_new if k_new is None else k_new,
                               self.v_new if v_new is None else v_new, self.lens if lens is None else lens, self.table, self.kd,
                               self.vd, self.cos, self.sin, self.interleaved)

    def q_rotated(self, start, per_row):
        if self.cos is None:
            return self.Q
        pos = start.long()[:, None, None] + (torch.arange(self.Q.shape[2])[None, None, :] if per_row else 0)
        return fa.apply_rotary(self.Q, self.cos, self.sin, pos, self.interleaved)

    def dev(self, *names):
        out = []
        for n in names:
            t = getattr(self, n) if isinstance(n, str) else n
            out.append(None if t is None else t.to(DEV))
        return out


def same(a, b):
    return torch.equal(bits(a.cpu()), bits(b.cpu()))


def run_fused(p, causal, window, n, variant, k_new=None, v_new=None):
    """The fused call on device copies of the problem -> (O, L, K_after, V_after) plus the device inputs, for the unchanged-inputs
    check."""
    Q, K, V, lens, table, kd, vd, cos, sin = p.dev("Q", "K", "V", "lens", "table", "kd", "vd", "cos", "sin")
    kn, vn = p.dev(p.k_new if k_new is None else k_new, p.v_new if v_new is None else v_new)
    if k_new is not None:  # strided views: rebuild them on the device with the same strides
        kn = torch.empty_strided(k_new.shape, k_new.stride(), dtype=k_new.dtype, device=DEV).copy_(k_new)
        vn = torch.empty_strided(v_new.shape, v_new.stride(), dtype=v_new.dtype, device=DEV).copy_(v_new)
    before = [None if t is None else t.clone() for t in (Q, kn, vn, lens, table)]
    O, L = fa.flash_attention_kvcache_forward(Q, K, V, lens, DEV, causal=causal, window=window, scale=Q.shape[3] ** -0.5, num_splits=n,
                                              variant=variant, k_descale=kd, v_descale=vd, block_table=table, k_new=kn, v_new=vn,
                                              rotary_cos=cos, rotary_sin=sin, rotary_interleaved=p.interleaved)
    for was, now in zip(before, (Q, kn, vn, lens, table)):  # the inputs are not modified
        assert was is None or torch.equal(bits(was), bits(now))
    return O, L, K, V


def existing_call(p, Ke, Ve, new_lens, start, causal, window, n, variant):
    """The existing decode call on the expected cache, the restated lengths and apply_rotary(Q)."""
    per_row = causal or window is not None
    Qr, K, V, lens, table, kd, vd = p.dev(p.q_rotated(start, per_row), Ke, Ve, new_lens, "table", "kd", "vd")
    return fa.flash_attention_kvcache_forward(Qr, K, V, lens, DEV, causal=causal, window=window, scale=Qr.shape[3] ** -0.5, num_splits=n,
                                              variant=variant, k_descale=kd, v_descale=vd, block_table=table)


def check_fused(p, causal, window, n, variant, what, k_new=None, v_new=None):
    Ke, Ve, start, new_lens = p.expected()
    O, L, K, V = run_fused(p, causal, window, n, variant, k_new, v_new)
    assert same(K, Ke), (what, "K cache")
    assert same(V, Ve), (what, "V cache")
    O_ref, L_ref = existing_call(p, Ke, Ve, new_lens, start, causal, window, n, variant)
    assert not torch.isnan(O).any() and not torch.isnan(L).any(), what
    assert same(O, O_ref) and same(L, L_ref), (what, "O, L")
    return O, L, K, V


# (variant, dtype, fp8 cache, descales given, d, page_size (None: contiguous), H, H_kv, N_new, N_q, rotary_dim as a divisor of d (0: none),
#  interleaved, causal, window, num_splits)
CONFIGS = [
    ("mfma16", BF, None, False, 128, None, 8, 2, 1, 1, 1, False, False, None, 1),
    ("mfma16", F16, None, False, 64, None, 8, 2, 3, 3, 2, True, True, None, 3),
    ("mfma16", BF, None, False, 64, 64, 8, 2, 3, 1, 1, True, False, None, 3),
    ("mfma16", F16, None, False, 128, 64, 8, 2, 1, 3, 2, False, True, None, 1),
    ("mfma16", BF, None, False, 128, 64, 8, 2, 3, 3, 0, False, True, None, 3),
    ("mfma16", F16, None, False, 64, None, 8, 2, 3, 3, 1, False, False, (100, 0), 1),
    ("mfma16", BF, E4, True, 128, None, 8, 2, 3, 3, 1, False, True, None, 1),
    ("mfma16", F16, E5, True, 64, 64, 8, 2, 3, 1, 2, True, False, None, 3),
    ("mfma16", BF, E4, False, 64, 64, 8, 2, 1, 3, 0, False, True, None, 3),
    ("mfma16", BF, E5, False, 128, None, 8, 2, 3, 1, 1, True, False, None, 1),
    ("mfma16", BF, None, False, 128, 64, 4, 4, 3, 3, 1, False, True, None, 3),   # MHA
    ("mfma16", F16, None, False, 64, None, 8, 1, 3, 1, 1, True, False, None, 1),  # MQA
    ("generic", BF, None, False, 64, 16, 8, 2, 3, 3, 1, False, True, None, 3),
    ("generic", F16, None, False, 128, 16, 8, 2, 1, 1, 2, True, False, None, 1),
    ("generic", BF, None, False, 128, None, 8, 2, 3, 1, 2, False, False, None, 3),
    ("generic", F16, None, False, 64, None, 8, 2, 3, 3, 0, False, True, None, 1),
    ("generic", F32, None, False, 40, None, 8, 2, 3, 3, 1, False, True, None, 3),
    ("generic", F32, None, False, 40, 16, 8, 2, 3, 1, 2, True, False, None, 1),
    ("generic", F32, None, False, 40, 16, 8, 2, 1, 3, 0, False, True, (100, 0), 3),
    ("generic", BF, E4, True, 64, 16, 8, 2, 3, 3, 2, False, False, (100, 0), 3),
    ("generic", BF, E5, True, 128, None, 8, 2, 1, 1, 0, False, False, None, 1),
    ("generic", F16, E4, False, 64, 16, 8, 2, 3, 1, 1, True, True, None, 1),
    ("generic", F16, E5, False, 128, 64, 8, 1, 3, 3, 1, False, True, None, 3),    # MQA, matrix-form page size on the VALU form
    ("generic", F64, None, False, 40, None, 4, 4, 3, 3, 2, True, True, None, 1),  # beyond the issue's list: f64 is computed in f64
]


def test_configs_cover_the_issue():
    m = [c for c in CONFIGS if c[0] == "mfma16"]
    g = [c for c in CONFIGS if c[0] == "generic"]
    for cs in (m, g):
        assert {c[1] for c in cs} >= {BF, F16} and {c[4] for c in cs} >= {64, 128} and {c[2] for c in cs} == {None, E4, E5}
        assert {(c[8], c[9]) for c in cs} == {(1, 1), (1, 3), (3, 1), (3, 3)}
        assert {c[10] for c in cs} == {0, 1, 2} and {c[11] for c in cs} == {False, True} and {c[12] for c in cs} == {False, True}
        assert {c[14] for c in cs} == {1, 3} and any(c[13] is not None for c in cs)
        assert {c[3] for c in cs if c[2] is not None} == {False, True}
        assert any(c[7] == 1 for c in cs) and any(c[5] is None for c in cs)
    assert any(c[6] == c[7] for c in CONFIGS)  # MHA
    assert {c[5] for c in m} == {None, 64} and {c[5] for c in g} >= {None, 16}
    assert any(c[1] == F32 and c[4] == 40 for c in g)
    assert {n for P in (16, 64) for ls in length_sets(P) for n in ls} == {0, 1, 15, 16, 62, 63, 64, 127, CAP - 3, CAP - 1, CAP}


@pytest.mark.parametrize("idx", range(len(CONFIGS)))
def test_cache_and_output_bit_equal_to_the_restatement(idx):
    variant, dtype, kv, descales, d, P, H, H_kv, N_new, N_q, rdiv, inter, causal, window, n = CONFIGS[idx]
    for lens in length_sets(P):
        p = Problem(dtype, kv, descales, d, P, H, H_kv, N_new, N_q, d // rdiv if rdiv else 0, inter, lens, seed=100 * idx + lens[1])
        O, L, _, _ = check_fused(p, causal, window, n, variant, (CONFIGS[idx], lens))
        assert O.shape == p.Q.shape and L.shape == p.Q.shape[:3] and O.dtype == dtype and L.dtype == dtype


def strided(t):
    """The same values as a d-strided view (every second column of a tensor twice as wide): forces the element path."""
    wide = torch.zeros(*t.shape[:-1], 2 * t.shape[-1], dtype=t.dtype)
    wide[..., ::2] = t
    return wide[..., ::2]


@pytest.mark.parametrize("dtype,kv,d,P,rdiv,inter", [(BF, None, 128, None, 1, False), (F16, None, 64, 64, 2, True), (BF, E4, 64, 16, 1, True),
                                                      (F16, E5, 128, None, 2, False), (BF, None, 64, 16, 0, False),
                                                      (BF, E5, 128, 64, 0, False)])
def test_vector_path_and_element_path_give_the_same_bits(dtype, kv, d, P, rdiv, inter):
    """k_new / v_new contiguous (vector path) and as d-strided views, or as flash-attn's (B, N_new, H_kv, d) layout: one result."""
    lens = length_sets(P)[0]
    p = Problem(dtype, kv, True, d, P, 8, 2, 3, 3, d // rdiv if rdiv else 0, inter, lens, seed=d + (P or 0))
    variant = "mfma16" if P != 16 else "generic"
    ref = check_fused(p, True, None, 3, variant, "contiguous")
    kn, vn = strided(p.k_new), strided(p.v_new)
    assert kn.stride(3) == 2 and torch.equal(kn, p.k_new)
    out = check_fused(p, True, None, 3, variant, "d-strided", kn, vn)
    nhd = lambda t: t.transpose(1, 2).contiguous().transpose(1, 2)
    out2 = check_fused(p, True, None, 3, variant, "(B, N_new, H_kv, d) storage", nhd(p.k_new), nhd(p.v_new))
    for o in (out, out2):
        for a, b in zip(ref, o):
            assert same(a, b)


@pytest.mark.parametrize("dtype,kv,d,P,N_new", [(BF, None, 128, None, 3), (F16, E4, 64, 64, 3), (F32, None, 40, 16, 3), (BF, E5, 128, 16, 1),
                                                 (BF, None, 64, 64, 40)])
def test_kvcache_append_alone(dtype, kv, d, P, N_new):
    """The cache update without Q: the returned lengths and the whole cache equal the restatement; N_new = 40 runs more than one
    token block and crosses pages."""
    for lens in length_sets(P):
        p = Problem(dtype, kv, True, d, P, 8, 2, N_new, 1, d // 2 if d != 40 else 40, False, lens, seed=N_new + d)
        Ke, Ve, _, new_lens = p.expected()
        K, V, kn, vn, lens_d, table, kd, vd, cos, sin = p.dev("K", "V", "k_new", "v_new", "lens", "table", "kd", "vd", "cos", "sin")
        got = fa.kvcache_append(K, V, kn, vn, lens_d, k_descale=kd, v_descale=vd, block_table=table, rotary_cos=cos, rotary_sin=sin)
        assert got.dtype == torch.int32 and got.shape == (4,) and torch.equal(got.cpu(), new_lens)
        assert torch.equal(lens_d.cpu(), p.lens)
        assert same(K, Ke) and same(V, Ve), (dtype, kv, P, lens)


def arena(shape, dtype, value=77):
    """A tensor inside a canary arena: (view, whole arena as bytes, byte range of the view)."""
    pad = 4096
    numel = math.prod(shape)
    size = torch.empty(0, dtype=dtype).element_size()
    whole = torch.full((numel * size + 2 * pad,), value, dtype=torch.uint8, device=DEV)
    return whole[pad:pad + numel * size].view(dtype).view(shape), whole, slice(pad, pad + numel * size)


def canaries_intact(whole, sl, value=77):
    return bool((whole[:sl.start] == value).all()) and bool((whole[sl.stop:] == value).all())


@pytest.mark.parametrize("variant,dtype,kv,P", [("mfma16", BF, None, 64), ("generic", F16, E4, 16), ("mfma16", BF, E5, None)])
def test_canaries_around_every_buffer_the_call_writes(variant, dtype, kv, P):
    B, H, H_kv, N_new, N_q, d, n = 4, 8, 2, 3, 3, 64, 3
    p = Problem(dtype, kv, True, d, P, H, H_kv, N_new, N_q, d, False, length_sets(P)[0], seed=31)
    Ke, Ve, start, new_lens = p.expected()
    Q, kn, vn, lens, table, kd, vd, cos, sin = p.dev("Q", "k_new", "v_new", "lens", "table", "kd", "vd", "cos", "sin")
    K, K_all, K_sl = arena(p.K.shape, p.K.dtype)
    V, V_all, V_sl = arena(p.V.shape, p.V.dtype)
    bits(K).copy_(bits(p.K))
    bits(V).copy_(bits(p.V))
    q_rot, q_all, q_sl = arena(Q.shape, dtype)
    out, out_all, out_sl = arena((B,), torch.int32)
    O, O_all, O_sl = arena(Q.shape, dtype)
    L, L_all, L_sl = arena(Q.shape[:3], dtype)
    ws, ws_all, ws_sl = arena((_lib.kvcache_workspace_bytes(B, H, N_q, d, n) // 4,), torch.float32)
    enum = convert_triton_dtype(dtype)
    _lib.fa2_fwd_kvcache_append(Q, K, V, O, L, kn, vn, lens, out, enum, convert_triton_dtype(p.K.dtype), block_table=table,
                                k_descale=kd, v_descale=vd, rotary_cos=cos, rotary_sin=sin, q_rot=q_rot, causal=True, scale=d ** -0.5,
                                num_splits=n, workspace=ws, variant=_lib.KVCACHE_VARIANTS[variant])
    torch.cuda.synchronize()
    for whole, sl in ((K_all, K_sl), (V_all, V_sl), (q_all, q_sl), (out_all, out_sl), (O_all, O_sl), (L_all, L_sl), (ws_all, ws_sl)):
        assert canaries_intact(whole, sl)
    assert same(K, Ke) and same(V, Ve) and torch.equal(out.cpu(), new_lens)
    assert same(q_rot, p.q_rotated(start, True))
    O_ref, L_ref = existing_call(p, Ke, Ve, new_lens, start, True, None, n, variant)
    assert same(O, O_ref) and same(L, L_ref)


@pytest.mark.parametrize("entry", [-1, INT_MAX])
def test_a_wild_table_entry_at_the_page_being_written_stays_inside_the_pool(entry):
    """Sequence 0's entry for the page it appends into is wild; sequence 1 is full and writes nothing.  Required: the canaries are
    intact and every pool byte that differs from before lies in the page the entry is clamped to."""
    P, d = 16, 64
    p = Problem(BF, None, False, d, P, 8, 2, 3, 1, d, False, [20, CAP], seed=41)
    p.table[0, 1] = entry
    kn, vn, lens, table, cos, sin = p.dev("k_new", "v_new", "lens", "table", "cos", "sin")
    K, K_all, K_sl = arena(p.K.shape, BF)
    V, V_all, V_sl = arena(p.V.shape, BF)
    bits(K).copy_(bits(p.K))
    bits(V).copy_(bits(p.V))
    got = fa.kvcache_append(K, V, kn, vn, lens, block_table=table, rotary_cos=cos, rotary_sin=sin)
    torch.cuda.synchronize()
    assert canaries_intact(K_all, K_sl) and canaries_intact(V_all, V_sl)
    assert got.tolist() == [23, CAP]
    page = 0 if entry < 0 else p.K.shape[0] - 1
    for pool, was in ((K, p.K), (V, p.V)):
        changed = (bits(pool.cpu()) != bits(was)).flatten(1).any(1).nonzero().view(-1).tolist()
        assert changed in ([page], []), changed
    Ke, Ve, _, _ = p.expected()  # the restatement clamps like the kernel
    assert same(K, Ke) and same(V, Ve)


@pytest.mark.parametrize("variant,dtype,kv,P", [("mfma16", BF, None, 64), ("generic", F16, E4, 16), ("generic", F32, None, None)])
def test_two_steps_in_a_row(variant, dtype, kv, P):
    """Step 2 takes step 1's new_seqlens; the final cache and O equal one restated run, and the same fused call repeated from the
    same initial state gives the same bits."""
    d = 40 if dtype == F32 else 64
    p = Problem(dtype, kv, True, d, P, 8, 2, 3, 1, d, True, [1, 62, CAP - 4, 127], seed=53, steps=2)
    g = torch.Generator().manual_seed(54)
    k2, v2 = ((torch.randn(4, 2, 3, d, generator=g) * 0.5).to(dtype) for _ in range(2))
    # restated: two appends in a row, then the existing call
    K1, V1, _, lens1 = p.expected()
    K2, V2, start2, lens2 = p.expected(K1, V1, lens1, k2, v2)
    K, V, kn, vn, lens, table, kd, vd, cos, sin, Q = p.dev("K", "V", "k_new", "v_new", "lens", "table", "kd", "vd", "cos", "sin", "Q")
    k2d, v2d = p.dev(k2, v2)
    got1 = fa.kvcache_append(K, V, kn, vn, lens, k_descale=kd, v_descale=vd, block_table=table, rotary_cos=cos, rotary_sin=sin,
                             rotary_interleaved=True)
    assert torch.equal(got1.cpu(), lens1) and same(K, K1) and same(V, V1)
    outs = []
    for _ in range(2):  # the fused step 2, twice from the same state
        Kc, Vc = K.clone(), V.clone()
        O, L = fa.flash_attention_kvcache_forward(Q, Kc, Vc, got1, DEV, causal=False, scale=d ** -0.5, num_splits=3, variant=variant,
                                                  k_descale=kd, v_descale=vd, block_table=table, k_new=k2d, v_new=v2d, rotary_cos=cos,
                                                  rotary_sin=sin, rotary_interleaved=True)
        assert same(Kc, K2) and same(Vc, V2)
        outs.append((O, L))
    assert same(outs[0][0], outs[1][0]) and same(outs[0][1], outs[1][1])
    O_ref, L_ref = existing_call(p, K2, V2, lens2, start2, False, None, 3, variant)
    assert same(outs[0][0], O_ref) and same(outs[0][1], L_ref)
