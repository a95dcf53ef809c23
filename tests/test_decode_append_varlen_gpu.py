"""The packed (ragged) KV-cache append on the GPU (fa2_kvcache_append_varlen, fa2_fwd_kvcache_varlen_append).  The yardstick
throughout is BIT-EQUALITY through integer views: the whole cache after the call equals tests/decode_append_restatement.py's
expected_append applied sequence by sequence on the CPU (sequence b's rows of the packed tensors, its length, table row and
descales; the cache or pool carried from one sequence to the next) -- which also proves that no other byte moved -- and O, L of the
fused call equal the existing packed-query call's on that restated cache.  No arithmetic is restated here and nothing has a
tolerance.

The initial cache holds ordinary data below the lengths and a seeded random bit pattern, NaN encodings included, past them; pools
hold spare pages under a seeded permutation and table entries of pages the append does not touch are -1 / 2^31 - 1; rows of the
packed tensors outside every sequence hold NaN.

One offsets array cannot put unowned rows between two sequences except as the surplus of a span longer than max_seqlen_new
(cu[b + 1] is both the end of b's span and the start of b + 1), so the gap of the offsets tests sits behind the 70-row sequence,
whose span is 72 rows under max_seqlen_new = 70, and a second case leaves 2 rows in front of the first offset."""
import math

import pytest
import torch

import flash_attention_dlrs_amd as fa
from flash_attention_dlrs_amd import _lib
from flash_attention_dlrs_amd.flash_attention_torch import convert_triton_dtype
from decode_append_restatement import INT_VIEW, bits, expected_append, new_lengths

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF, F16, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64
E4, E5 = torch.float8_e4m3fn, torch.float8_e5m2
INT_MAX = 2 ** 31 - 1
CAP = 256
SPARE = 3  # pool pages no table names
S_ROT = CAP + 8

N_NEW = [0, 1, 3, 16, 17, 70, 1, 5]
LENS = [100, 0, 63, 15, 240, 186, 256, 254]
LENS_CLAMPS = [-5, 300, 16, 64, 127, 0, 255, 1]  # the clamps at both ends


def test_the_batch_holds_the_cases_it_is_there_for():
    assert len(N_NEW) == len(LENS) == len(LENS_CLAMPS) == 8 and sum(N_NEW) == 113 and max(N_NEW) == 70
    pairs = list(zip(LENS, N_NEW))
    assert (100, 0) in pairs                      # an empty sequence whose length is still written
    assert (0, 1) in pairs                        # a token into an empty cache
    assert (63, 3) in pairs and 63 % 16 == 15 and 63 % 64 == 63 and 63 + 3 > 64   # a straddle of a 16- and a 64-key page edge
    assert (15, 16) in pairs and (15 + 16) // 16 > 15 // 16                        # a run across 16-key pages
    assert (240, 17) in pairs and CAP - 240 == 16 and (254, 5) in pairs and CAP - 254 == 2   # partly dropped tails
    assert (186, 70) in pairs and 186 + 70 == CAP                                  # a fill to exactly the last row
    assert (256, 1) in pairs                                                       # a wholly dropped sequence
    cu = cu_of(N_NEW).tolist()
    assert len({c // 16 for c in cu[:4]}) == 1    # several sequences inside one block of 16 packed rows
    assert min(LENS_CLAMPS) < 0 and max(LENS_CLAMPS) > CAP


def cu_of(spans, first=0):
    return torch.tensor([first] + spans, dtype=torch.int64).cumsum(0).to(torch.int32)


def random_bits(shape, dtype, g):
    """A seeded random bit pattern in `dtype` (NaN and inf encodings included), on the CPU."""
    it = INT_VIEW[torch.empty(0, dtype=dtype).element_size()]
    info = torch.iinfo(it)
    return torch.randint(info.min, info.max, shape, generator=g, dtype=torch.int64).to(it).view(dtype)


class Packed:
    """One packed append problem on the CPU: Q and the new tokens (packed over cu), the initial cache (or pool and table),
    descales, rotary tables.  `spans` are the rows cu gives each sequence; sequence b takes min(spans[b], max_new) of them."""

    def __init__(self, dtype, kv, descales, d, P, H, H_kv, rd, interleaved, lens, spans, seed, max_new=None, first=0, tail=0):
        g = torch.Generator().manual_seed(seed)
        B = len(lens)
        self.dtype, self.P, self.interleaved, self.B = dtype, P, interleaved, B
        self.lens = torch.tensor(lens, dtype=torch.int32)
        self.cu = cu_of(spans, first)
        self.total = int(self.cu[-1]) + tail
        self.max_new = max(max(spans), 1) if max_new is None else max_new
        self.s = self.cu[:-1].tolist()
        self.n = [min(n, self.max_new) for n in spans]
        self.live = torch.zeros(self.total, dtype=torch.bool)
        for s, n in zip(self.s, self.n):
            self.live[s:s + n] = True
        self.Q = (torch.randn(self.total, H, d, generator=g) * 0.5).to(dtype)
        self.k_new = (torch.randn(self.total, H_kv, d, generator=g) * 0.5).to(dtype)
        self.v_new = (torch.randn(self.total, H_kv, d, generator=g) * 0.5).to(dtype)
        for t in (self.Q, self.k_new, self.v_new):  # rows outside every sequence: not to be read
            t[~self.live] = float("nan")
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
                used = -(-min(min(max(n, 0), CAP) + self.n[b], CAP) // P)
                for i in range(used, mb):
                    self.table[b, i] = (-1, INT_MAX)[(i - used) % 2]
        self.K, self.V = K, V

    def expected(self):
        """(K, V, start, seqlens_out): expected_append, one sequence after the other."""
        K, V = self.K.clone(), self.V.clone()
        starts, outs = [], []
        for b in range(self.B):
            s, n = self.s[b], self.n[b]
            lens_b = self.lens[b:b + 1]
            if n == 0:
                start, out = new_lengths(lens_b, 0, CAP)
            else:
                kn, vn = (t[s:s + n].transpose(0, 1)[None] for t in (self.k_new, self.v_new))
                kd, vd = (None if t is None else t[b:b + 1] for t in (self.kd, self.vd))
                if self.table is None:
                    Kb, Vb, start, out = expected_append(K[b:b + 1], V[b:b + 1], kn, vn, lens_b, None, kd, vd, self.cos, self.sin,
                                                         self.interleaved)
                    bits(K)[b:b + 1], bits(V)[b:b + 1] = bits(Kb), bits(Vb)
                else:
                    K, V, start, out = expected_append(K, V, kn, vn, lens_b, self.table[b:b + 1], kd, vd, self.cos, self.sin,
                                                       self.interleaved)
            starts.append(start)
            outs.append(out)
        return K, V, torch.cat(starts), torch.cat(outs)

    def q_rotated(self, start, per_row):
        """apply_rotary(Q) at start(b) + i (per_row) or start(b), clamped as the kernel clamps; rows outside every sequence as they are."""
        if self.cos is None:
            return self.Q
        pos = torch.zeros(self.total, dtype=torch.int64)
        for b, (s, n) in enumerate(zip(self.s, self.n)):
            pos[s:s + n] = int(start[b]) + (torch.arange(n) if per_row else 0)
        return fa.apply_rotary(self.Q, self.cos, self.sin, pos[:, None], self.interleaved)

    def dev(self, *names):
        out = []
        for n in names:
            t = getattr(self, n) if isinstance(n, str) else n
            out.append(None if t is None else t.to(DEV))
        return out


def same(a, b):
    return torch.equal(bits(a.cpu()), bits(b.cpu()))


def on_device(t):
    """A CPU tensor on the device with the same strides."""
    return torch.empty_strided(t.shape, t.stride(), dtype=t.dtype, device=DEV).copy_(t)


def wide_slice(t):
    """The same values as a slice of a wider (total, H_kv + 1, d + 8) tensor: token and head strides stay multiples of 8."""
    wide = torch.full((t.shape[0], t.shape[1] + 1, t.shape[2] + 8), float("nan"), dtype=t.dtype)
    wide[:, :t.shape[1], :t.shape[2]] = t
    return wide[:, :t.shape[1], :t.shape[2]]


def misaligned(t):
    """The same values with a token stride of H_kv * d + 4 elements, which breaks the vector path's alignment."""
    total, hk, d = t.shape
    buf = torch.full((total, hk * d + 4), float("nan"), dtype=t.dtype)
    view = buf[:, :hk * d].view(total, hk, d)
    view.copy_(t)
    return view


LAYOUTS = {"contiguous": lambda t: t, "wide": wide_slice, "misaligned": misaligned}


def run_append(p, layout="contiguous", K=None, V=None):
    """kvcache_append_varlen on device copies of the problem -> (K_after, V_after, new_seqlens); the inputs must come out unchanged."""
    lens, cu, table, kd, vd, cos, sin = p.dev("lens", "cu", "table", "kd", "vd", "cos", "sin")
    K, V = p.dev(p.K if K is None else K, p.V if V is None else V)
    kn, vn = (on_device(LAYOUTS[layout](t)) for t in (p.k_new, p.v_new))
    before = [None if t is None else t.clone() for t in (kn, vn, lens, cu, table)]
    got = fa.kvcache_append_varlen(K, V, kn, vn, cu, p.max_new, lens, k_descale=kd, v_descale=vd, block_table=table, rotary_cos=cos,
                                   rotary_sin=sin, rotary_interleaved=p.interleaved)
    for was, now in zip(before, (kn, vn, lens, cu, table)):
        assert was is None or torch.equal(bits(was), bits(now))
    return K, V, got


def check_append(p, what, layout="contiguous"):
    Ke, Ve, _, new_lens = p.expected()
    K, V, got = run_append(p, layout)
    assert got.dtype == torch.int32 and got.shape == (p.B,) and torch.equal(got.cpu(), new_lens), (what, got.tolist(), new_lens.tolist())
    assert same(K, Ke), (what, "K cache")
    assert same(V, Ve), (what, "V cache")
    return K, V, got


# (dtype, fp8 cache, descales given, d, page_size (None: contiguous), H_kv, rotary_dim (0: none), interleaved, layout of k_new / v_new)
CASES = [
    (BF, None, False, 128, None, 3, 128, False, "contiguous"),
    (F16, None, False, 128, 16, 1, 64, True, "contiguous"),
    (BF, None, False, 64, 64, 3, 64, True, "wide"),
    (F16, None, False, 64, 128, 1, 32, False, "contiguous"),
    (BF, None, False, 128, 128, 3, 0, False, "wide"),
    (BF, None, False, 128, 16, 3, 24, False, "contiguous"),          # rotary_dim % 16 != 0: the element path
    (F16, None, False, 64, None, 1, 24, True, "contiguous"),
    (BF, None, False, 128, 64, 3, 128, False, "misaligned"),         # the element path by the token stride
    (F16, E4, True, 64, 16, 1, 64, False, "misaligned"),
    (F32, None, False, 128, None, 3, 64, True, "contiguous"),        # the element path by the dtype
    (F32, None, False, 128, 64, 1, 0, False, "wide"),
    (F64, None, False, 128, 16, 3, 128, False, "contiguous"),
    (BF, None, False, 40, None, 3, 40, False, "contiguous"),         # d % 8 != 0
    (BF, None, False, 40, 16, 1, 20, True, "contiguous"),
    (BF, E4, True, 128, None, 3, 64, False, "contiguous"),
    (F16, E5, True, 64, 64, 1, 64, True, "wide"),
    (BF, E4, False, 64, 128, 3, 0, False, "contiguous"),
    (F16, E5, False, 128, 16, 3, 128, False, "contiguous"),
    (BF, E5, True, 40, None, 1, 24, True, "contiguous"),             # an fp8 cache on the element path
]


def test_cases_cover_the_issue():
    vec = [c for c in CASES if c[0] in (BF, F16) and c[3] % 8 == 0 and c[6] % 16 == 0 and c[8] != "misaligned"]
    assert {(c[0], c[3]) for c in vec} >= {(BF, 128), (BF, 64), (F16, 128), (F16, 64)}
    assert any(c[0] == F32 and c[3] == 128 for c in CASES) and any(c[0] == F64 and c[3] == 128 for c in CASES)
    assert any(c[0] == BF and c[3] == 40 for c in CASES)
    assert {(c[1], c[2]) for c in CASES if c[1] is not None} == {(E4, True), (E4, False), (E5, True), (E5, False)}
    assert {c[4] for c in CASES} == {None, 16, 64, 128} and {c[5] for c in CASES} == {1, 3}
    assert {0 if c[6] == 0 else c[3] // c[6] if c[6] != 24 else 24 for c in CASES} >= {0, 1, 2, 24}
    assert {c[7] for c in CASES if c[6]} == {False, True} and {c[8] for c in CASES} == set(LAYOUTS)


@pytest.mark.parametrize("idx", range(len(CASES)))
def test_cache_and_lengths_bit_equal_to_the_restatement(idx):
    dtype, kv, descales, d, P, H_kv, rd, inter, layout = CASES[idx]
    for k, lens in enumerate((LENS, LENS_CLAMPS)):
        p = Packed(dtype, kv, descales, d, P, H_kv, H_kv, rd, inter, lens, N_NEW, seed=10 * idx + k)
        assert p.total == 113 and p.max_new == 70
        check_append(p, (CASES[idx], lens), layout)


def test_strided_layouts_are_what_they_claim():
    t = torch.randn(5, 3, 128).to(BF)
    w, m = wide_slice(t), misaligned(t)
    assert w.stride() == (4 * 136, 136, 1) and torch.equal(w, t)
    assert m.stride() == (3 * 128 + 4, 128, 1) and m.stride(0) % 8 != 0 and torch.equal(m, t)
    assert on_device(m).stride() == m.stride()


# (what, spans of cu, max_seqlen_new, rows in front of the first offset, rows behind the last, total_new, rows in no sequence)
OFFSETS = [
    ("a 2-row surplus behind the 70-row sequence and 4 rows behind the last offset", [0, 1, 3, 16, 17, 72, 1, 5], 70, 0, 4, 119, 6),
    ("2 rows in front of the first offset", N_NEW, 70, 2, 0, 115, 2),
    ("max_seqlen_new = 16", N_NEW, 16, 0, 0, 113, 1 + 54),
]


@pytest.mark.parametrize("dtype,kv,d,P,rd", [(BF, None, 128, None, 128), (F16, E4, 64, 16, 32), (F32, None, 40, 64, 24)])
@pytest.mark.parametrize("what,spans,max_new,first,tail,total,dead", OFFSETS, ids=[o[0] for o in OFFSETS])
def test_rows_outside_every_sequence_are_not_read(what, spans, max_new, first, tail, total, dead, dtype, kv, d, P, rd):
    p = Packed(dtype, kv, True, d, P, 2, 2, rd, False, LENS, spans, seed=7, max_new=max_new, first=first, tail=tail)
    assert p.total == total and int((~p.live).sum()) == dead and torch.isnan(p.k_new[~p.live].float()).all()
    if max_new == 16:
        assert p.n[4] == 16 and p.n[5] == 16 and LENS[4] + 16 == CAP  # 240 + 16 fills exactly
    _, _, got = check_append(p, what)
    assert got.tolist() == [min(min(max(n, 0), CAP) + k, CAP) for n, k in zip(LENS, p.n)]


@pytest.mark.parametrize("P", [None, 16])
def test_two_empty_sequences_at_one_offset(P):
    p = Packed(BF, None, False, 64, P, 2, 2, 64, True, [10, CAP, 250, 0, 30], [0, 0, 5, 0, 4], seed=11)
    assert p.cu.tolist() == [0, 0, 0, 5, 5, 9]
    _, _, got = check_append(p, "cu = [0, 0, 0, 5, 5, 9]")
    assert got.tolist() == [10, CAP, 255, 0, 34]


@pytest.mark.parametrize("dtype,kv,P,rd", [(BF, None, None, 64), (F16, None, 16, 32), (BF, E4, 64, 64), (F32, None, 16, 24)])
def test_a_uniform_batch_equals_the_fixed_append(dtype, kv, P, rd):
    """n_new = 3 everywhere: the packed call against the existing kvcache_append on the same data reshaped, cache and lengths."""
    d = 40 if dtype == F32 else 64
    p = Packed(dtype, kv, True, d, P, 2, 2, rd, False, [0, 63, CAP - 1, CAP, 15, 127], [3] * 6, seed=13)
    K, V, got = run_append(p)
    lens, table, kd, vd, cos, sin, K2, V2 = p.dev("lens", "table", "kd", "vd", "cos", "sin", "K", "V")
    kn, vn = (t.view(p.B, 3, 2, d).transpose(1, 2).to(DEV) for t in (p.k_new, p.v_new))
    got2 = fa.kvcache_append(K2, V2, kn, vn, lens, k_descale=kd, v_descale=vd, block_table=table, rotary_cos=cos, rotary_sin=sin)
    assert torch.equal(got, got2) and same(K, K2) and same(V, V2)
    assert not same(K, p.K)


def keys_of(cache, p, b):
    """Sequence b's part of a cache after a call: its batch row, or the pool pages its table row names (entries inside the pool)."""
    if p.table is None:
        return cache[b].cpu()
    pages = [int(e) for e in p.table[b] if 0 <= int(e) < cache.shape[0]]
    return cache.cpu()[pages]


@pytest.mark.parametrize("dtype,kv,P", [(BF, None, None), (F16, E5, 64)])
def test_every_sequence_alone_equals_its_rows_in_the_batch(dtype, kv, P):
    p = Packed(dtype, kv, True, 64, P, 2, 2, 64, False, LENS, N_NEW, seed=17)
    K, V, got = run_append(p)
    for b in range(p.B):
        one = Packed.__new__(Packed)
        one.__dict__.update(p.__dict__)
        one.B, one.lens, one.max_new = 1, p.lens[b:b + 1], max(p.n[b], 1)
        one.cu = torch.tensor([p.s[b], p.s[b] + p.n[b]], dtype=torch.int32)  # the same packed tensors, one sequence's span
        one.kd, one.vd = (None if t is None else t[b:b + 1] for t in (p.kd, p.vd))
        if P is None:
            one.K, one.V, one.table = p.K[b:b + 1], p.V[b:b + 1], None
        else:
            one.table = p.table[b:b + 1]
        K1, V1, got1 = run_append(one)
        assert got1.tolist() == [int(got[b])]
        if P is None:
            assert same(K1[0], K[b]) and same(V1[0], V[b]), b
        else:
            assert same(keys_of(K1, one, 0), keys_of(K, p, b)) and same(keys_of(V1, one, 0), keys_of(V, p, b)), b


def test_the_same_call_twice_gives_the_same_bits():
    p = Packed(BF, E4, True, 128, 16, 3, 3, 64, True, LENS, N_NEW, seed=19)
    a, b = run_append(p), run_append(p)
    assert all(same(x, y) for x, y in zip(a, b))


# ---- the fused call ----------------------------------------------------------------------------------------------------------------

def run_fused(p, causal, window, n, variant):
    Q, K, V, kn, vn, lens, cu, table, kd, vd, cos, sin = p.dev("Q", "K", "V", "k_new", "v_new", "lens", "cu", "table", "kd", "vd", "cos", "sin")
    before = [None if t is None else t.clone() for t in (Q, kn, vn, lens, cu, table)]
    O, L = fa.flash_attention_varlen_kvcache_forward(Q, K, V, cu, p.max_new, lens, DEV, causal=causal, window=window, scale=Q.shape[2] ** -0.5,
                                                     num_splits=n, variant=variant, k_descale=kd, v_descale=vd, block_table=table,
                                                     k_new=kn, v_new=vn, rotary_cos=cos, rotary_sin=sin, rotary_interleaved=p.interleaved)
    for was, now in zip(before, (Q, kn, vn, lens, cu, table)):
        assert was is None or torch.equal(bits(was), bits(now))
    return O, L, K, V


def existing_call(p, Ke, Ve, new_lens, start, causal, window, n, variant):
    """The existing packed-query call on the restated cache, the restated lengths and apply_rotary(Q)."""
    per_row = causal or window is not None
    Qr, K, V, lens, cu, table, kd, vd = p.dev(p.q_rotated(start, per_row), Ke, Ve, new_lens, "cu", "table", "kd", "vd")
    return fa.flash_attention_varlen_kvcache_forward(Qr, K, V, cu, p.max_new, lens, DEV, causal=causal, window=window,
                                                     scale=Qr.shape[2] ** -0.5, num_splits=n, variant=variant, k_descale=kd, v_descale=vd,
                                                     block_table=table)


# (H, H_kv, fp8 cache, page_size, rotary_dim, causal, window, num_splits, variant)
FUSED = [
    (8, 2, None, None, 64, True, None, 1, "auto"),
    (8, 2, None, None, 64, False, None, 3, "mfma16"),
    (8, 2, None, None, 0, False, (32, 0), 1, "generic"),
    (8, 2, None, 64, 32, True, None, 3, "auto"),
    (8, 2, None, 64, 64, False, (32, 0), 1, "mfma16"),
    (8, 2, None, 64, 0, False, None, 3, "generic"),
    (8, 2, E4, None, 64, True, None, 3, "generic"),
    (8, 2, E4, None, 64, False, (32, 0), 3, "auto"),
    (8, 2, E4, None, 0, False, None, 1, "mfma16"),
    (2, 2, None, None, 64, True, None, 3, "mfma16"),
    (2, 2, None, 64, 64, False, None, 1, "auto"),
    (2, 2, E4, None, 32, False, (32, 0), 1, "generic"),
    (2, 2, None, None, 64, False, None, 1, "generic"),
    (2, 2, None, 64, 0, True, None, 3, "generic"),
    (2, 2, E4, None, 64, True, None, 1, "auto"),
]


def test_fused_cases_cover_the_issue():
    for H in (8, 2):
        cs = [c for c in FUSED if c[0] == H]
        assert {(c[2], c[3]) for c in cs} == {(None, None), (None, 64), (E4, None)}
        assert {c[5] for c in cs} == {False, True} and any(c[6] == (32, 0) for c in cs)
        assert {c[7] for c in cs} == {1, 3} and {c[8] for c in cs} == {"auto", "mfma16", "generic"}
        assert any(c[4] == 0 for c in cs) and any(c[4] for c in cs)


@pytest.mark.parametrize("idx", range(len(FUSED)))
def test_fused_call_equals_the_existing_call_on_the_restated_cache(idx):
    H, H_kv, kv, P, rd, causal, window, n, variant = FUSED[idx]
    p = Packed(BF if idx % 2 else F16, kv, True, 64, P, H, H_kv, rd, bool(idx % 3 == 0), LENS, N_NEW, seed=200 + idx)
    Ke, Ve, start, new_lens = p.expected()
    O, L, K, V = run_fused(p, causal, window, n, variant)
    assert same(K, Ke) and same(V, Ve), (FUSED[idx], "cache")
    O_ref, L_ref = existing_call(p, Ke, Ve, new_lens, start, causal, window, n, variant)
    live = p.live.to(DEV)
    assert O.shape == p.Q.shape and L.shape == (H, p.total)
    assert not torch.isnan(O[live]).any() and not torch.isnan(L[:, live]).any()
    assert same(O[live], O_ref[live]) and same(L[:, live], L_ref[:, live]), (FUSED[idx], "O, L")


@pytest.mark.parametrize("kv,P,causal,n", [(None, None, True, 1), (None, 64, False, 3), (E4, None, True, 3), (None, None, False, 1)])
def test_a_uniform_fused_batch_equals_the_fixed_fused_call(kv, P, causal, n):
    """n_q = 2, g = 4: caches, O and L against flash_attention_kvcache_forward(..., k_new=, v_new=, rotary_cos=, rotary_sin=) at the same
    explicit num_splits."""
    B, H, H_kv, d, nq = 4, 8, 2, 64, 2
    p = Packed(BF, kv, True, d, P, H, H_kv, d, False, [0, 63, 200, CAP - 1], [nq] * B, seed=23)
    O, L, K, V = run_fused(p, causal, None, n, "auto")
    Q, K2, V2, lens, table, kd, vd, cos, sin = p.dev("Q", "K", "V", "lens", "table", "kd", "vd", "cos", "sin")
    kn, vn = (t.view(B, nq, H_kv, d).transpose(1, 2).to(DEV) for t in (p.k_new, p.v_new))
    O2, L2 = fa.flash_attention_kvcache_forward(Q.view(B, nq, H, d).transpose(1, 2), K2, V2, lens, DEV, causal=causal, scale=d ** -0.5,
                                                num_splits=n, k_descale=kd, v_descale=vd, block_table=table, k_new=kn, v_new=vn,
                                                rotary_cos=cos, rotary_sin=sin)
    assert same(K, K2) and same(V, V2)
    assert same(O.view(B, nq, H, d).transpose(1, 2).contiguous(), O2)
    assert same(L.view(H, B, nq).permute(1, 0, 2).contiguous(), L2)


# ---- canaries ----------------------------------------------------------------------------------------------------------------------

def arena(shape, dtype, value=77):
    """A tensor inside a canary arena: (view, whole arena as bytes, byte range of the view)."""
    pad = 4096
    numel = math.prod(shape)
    size = torch.empty(0, dtype=dtype).element_size()
    whole = torch.full((numel * size + 2 * pad,), value, dtype=torch.uint8, device=DEV)
    return whole[pad:pad + numel * size].view(dtype).view(shape), whole, slice(pad, pad + numel * size)


def canaries_intact(whole, sl, value=77):
    return bool((whole[:sl.start] == value).all()) and bool((whole[sl.stop:] == value).all())


@pytest.mark.parametrize("dtype,kv,P,per_row", [(BF, None, 64, True), (F16, E4, 16, False), (F32, None, None, True)])
def test_canaries_around_seqlens_out_and_q_rot(dtype, kv, P, per_row):
    """Through _lib: the arenas around seqlens_out and q_rot keep their canary, and so do the rows of q_rot outside every sequence
    (the surplus of the 72-row span, the rows behind the last offset)."""
    d, H, H_kv = (40 if dtype == F32 else 64), 4, 2
    _, spans, max_new, first, tail, total, dead = OFFSETS[0]
    p = Packed(dtype, kv, True, d, P, H, H_kv, d if dtype != F32 else 24, False, LENS, spans, seed=29, max_new=max_new, first=first, tail=tail)
    Ke, Ve, start, new_lens = p.expected()
    Q, K, V, kn, vn, lens, cu, table, kd, vd, cos, sin = p.dev("Q", "K", "V", "k_new", "v_new", "lens", "cu", "table", "kd", "vd", "cos", "sin")
    q_rot, q_all, q_sl = arena(Q.shape, dtype)
    out, out_all, out_sl = arena((p.B,), torch.int32)
    _lib.fa2_kvcache_append_varlen(K, V, kn, vn, cu, p.max_new, lens, out, convert_triton_dtype(dtype), convert_triton_dtype(p.K.dtype),
                                   block_table=table, k_descale=kd, v_descale=vd, rotary_cos=cos, rotary_sin=sin, Q=Q, q_rot=q_rot,
                                   q_pos_per_row=per_row)
    torch.cuda.synchronize()
    assert canaries_intact(q_all, q_sl) and canaries_intact(out_all, out_sl)
    assert torch.equal(out.cpu(), new_lens) and same(K, Ke) and same(V, Ve)
    rows = q_rot.cpu()
    assert int((~p.live).sum()) == dead and bool((rows[~p.live].contiguous().view(torch.uint8) == 77).all())
    assert same(rows[p.live], p.q_rotated(start, per_row)[p.live])
