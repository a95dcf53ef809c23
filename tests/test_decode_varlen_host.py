"""Variable-length (packed) queries over the KV cache (fa2_fwd_kvcache_varlen), the part that needs no GPU: the three exported
symbols, every argument error before any launch (fake pointers), the workspace formula, the split heuristic, the Python wrapper's
errors on CPU tensors -- and the CPU proof for tests/test_decode_varlen_probe_gpu.py: on the ragged batch that file runs, each
error a query-tiled kernel over packed rows can make (the mask taken from the position in the tile, the shift taken from
max_seqlen_q, a neighbour's cu_seqlens_q offset, a tile's key range one 64-key tile short at either end, the rows of a tile
transposed) breaks a bar of the exact-arithmetic probe (oracle/fa2_decode_probe.py) in every sequence whose truth it changes,
while the fp32 restatement of the split kernels breaks none.  The ragged helpers the GPU file shares live here."""
import ctypes
import functools
import os
import re
import subprocess

import pytest
import torch

from conftest import ROOT

import flash_attention_dlrs_amd as fa
from flash_attention_dlrs_amd import _lib
from flash_attention_dlrs_amd.flash_attention_wrappers import check_varlen_kvcache_args
from oracle import fa2_decode_probe as D
from oracle.fa2_bwd_arith import band

F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
SYMBOLS = ("fa2_fwd_kvcache_varlen", "fa2_kvcache_varlen_workspace_bytes", "fa2_kvcache_varlen_num_splits")

# ----------------------------------------------------------------------------- the ragged batch (tests/test_decode_varlen_gpu.py's)
S_K = 2560
H_KV = 2
MAX_Q = 300
N_Q = [0, 1, 2, 15, 16, 17, 63, 64, 65, 130, 1, 300]
N_K = [100, 0, 2, 16, 10, 65, 1000, 64, S_K, 200, 777, 2500]
B = len(N_Q)
CU = [0] + torch.tensor(N_Q).cumsum(0).tolist()
# (g, causal, window): tiles of 16, 8, 64, 32 and 4 query positions
PROBE_CONFIGS = [(4, True, None), (8, False, (100, 50)), (1, True, (64, 0)), (2, True, (0, 0)), (16, False, None)]
PLANTS = ("tile_local_mask", "shift_from_max", "neighbour_offset", "clip_first_tile", "clip_last_tile", "row_transposed")


def tile_q(g, max_q=MAX_Q):
    """query positions per workgroup of the matrix form"""
    return min(64 // g, max_q)


@functools.lru_cache(maxsize=None)
def ragged_cache(d, device=None):
    """the probe's K, V (B, H_kv, S_k, d) in float64 with decoys behind N_k(b)"""
    return D.probe_cache(d, lens=N_K, s_k=S_K, h_kv=H_KV, device=device)


def pack_rows(x, g, n_q):
    """(1, H_kv, R, ...) rows of the KV groups, r = hg n_q + i -> packed (n_q, H, ...)"""
    return D.to_heads(x, g, n_q)[0].transpose(0, 1)


def group_rows(x, g):
    """packed (n_q, H, ...) -> (1, H_kv, R, ...)"""
    return D.to_groups(x.transpose(0, 1).unsqueeze(0), g, x.shape[0])


def seq_queries(g, n_q, d, uniform, device=None):
    return D.probe_queries(g, n_q, d, uniform, B=1, h_kv=H_KV, device=device)


def packed_queries(g, d, uniform, device=None):
    """the probe's Q of every sequence, packed (total_q, H, d)"""
    return torch.cat([pack_rows(seq_queries(g, n, d, uniform, device), g, n) for n in N_Q if n])


def seq_keep(g, n_q, n_k, causal, window, plant=None, device=None):
    """(1, 1, R, S_k) visible (row, key) pairs of one sequence; plant: a mask or key-range error of a query-tiled kernel"""
    keep = D.decode_keep(g, n_q, causal, window, lens=[n_k], s_k=S_K, device=device)
    if plant is None:
        return keep
    base = keep[0, 0, :n_q].clone()                       # (n_q, S_k): the rows of one head
    tq = tile_q(g)
    if plant == "tile_local_mask":                        # the band's row taken at the position in the tile
        base = base[torch.arange(n_q, device=device) % tq]
    elif plant == "shift_from_max":                       # the bottom-right shift N_k - max_seqlen_q
        m = band(MAX_Q, n_k, causal, window, device)
        base = torch.zeros_like(base)
        base[:, :n_k] = m[:n_q]
    else:
        for q0 in range(0, n_q, tq):                      # the 64-key tiles the band of the tile's rows touches
            rows = base[q0:q0 + tq]
            cols = torch.nonzero(rows.any(0)).flatten()
            if cols.numel():
                first, last = int(cols[0]), int(cols[-1])
                if plant == "clip_first_tile":
                    rows[:, first // 64 * 64:first // 64 * 64 + 64] = False
                elif plant == "clip_last_tile":
                    rows[:, last // 64 * 64:last + 1] = False
                else:
                    raise ValueError(plant)
    return base.repeat(g, 1).view(1, 1, g * n_q, S_K)


def transposed_rows(g, n_q):
    """source row of each of the R rows when row hg tq + i of a query tile is read as i g + hg"""
    tq = tile_q(g)
    src = torch.empty(g * n_q, dtype=torch.long)
    for q0 in range(0, n_q, tq):
        t = min(tq, n_q - q0)
        for hg in range(g):
            for i in range(t):
                s = i * g + hg
                src[hg * n_q + q0 + i] = (s // t) * n_q + q0 + s % t
    return src


def ragged_truth(g, d, causal, window, uniform, dtype, plant=None, device=None):
    """[(Q_b, keep_b, O_b, L_b) or None] per sequence in the (1, H_kv, R, ...) layout: the fp64 truth, or that of a planted error"""
    K, V = ragged_cache(d, device)
    Qp = packed_queries(g, d, uniform, device)
    out = []
    for b, (nq, nk) in enumerate(zip(N_Q, N_K)):
        if nq == 0:
            out.append(None)
            continue
        Q = seq_queries(g, nq, d, uniform, device)
        if plant == "neighbour_offset":                   # the rows read from the next sequence's offset on
            tok = (CU[b + 1] + torch.arange(nq, device=device)) % Qp.shape[0]
            Q = group_rows(Qp[tok], g)
        keep = seq_keep(g, nq, nk, causal, window, plant if plant not in ("neighbour_offset", "row_transposed") else None, device)
        O, L = D.truth(Q, K[b:b + 1], V[b:b + 1], keep, dtype)
        if plant == "row_transposed":
            src = transposed_rows(g, nq).to(O.device)
            O, L = O[:, :, src], L[:, :, src]
        out.append((Q, keep, O, L))
    return out


# ----------------------------------------------------------------------------- symbols, argument errors, formulas
def test_symbols_exported_declared_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fa2_fwd.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exports = open(os.path.join(ROOT, "flash_attention_dlrs_amd", "csrc", "fa2_exports.map")).read()
    for name in SYMBOLS:
        assert name in _lib.SYMBOLS
        assert re.search(rf"\b{name}\s*\(", header), name
        assert re.search(rf"\bT {name}\b", out), name
        assert re.search(rf"\b{name};", exports), name
    assert callable(_lib.fa2_fwd_kvcache_varlen) and callable(fa.flash_attention_varlen_kvcache_forward)
    assert "flash_attention_varlen_kvcache_forward" in fa.__all__


def _call(ptr=0x1000, cu=0x5000, table=None, table_stride=None, B=2, H=8, H_kv=2, total_q=40, max_q=32, S_k=512, num_blocks=32,
          page_size=64, max_blocks=8, d=64, dtype=_lib.FA2_DTYPE_BF16, kv_dtype=None, num_splits=1, ws=None, ws_bytes=0, variant=0,
          q_strides=None, k_strides=None, l_stride=None, kd=None, kd_strides=None, window=(-1, -1), q_null=False, o_null=False):
    i64 = lambda v: None if v is None else (ctypes.c_int64 * len(v))(*v)
    qs = q_strides or (H * d, d, 1)
    rows = page_size if table else S_k
    ks = k_strides or (H_kv * rows * d, rows * d, d, 1)
    rc = _lib.lib().fa2_fwd_kvcache_varlen(ptr, ptr, ptr, ptr, ptr, None if q_null else i64(qs), i64(ks), i64(ks),
                                           None if o_null else i64(qs), total_q if l_stride is None else l_stride, cu, None, table,
                                           max_blocks if table_stride is None else table_stride, kd, None, i64(kd_strides), None, B, H,
                                           H_kv, total_q, max_q, S_k, num_blocks, page_size, max_blocks, d, dtype,
                                           dtype if kv_dtype is None else kv_dtype, 0, 1.0, window[0], window[1], num_splits, ws,
                                           ws_bytes, variant, None)
    return rc, _lib.lib().fa2_last_error().decode()


PAGED = dict(table=0x4000)


@pytest.mark.parametrize("kwargs,code,needle", [
    # the packed queries
    (dict(cu=None), -1, "cu_seqlens_q"), (dict(total_q=0), -1, "total_q"), (dict(total_q=-5), -1, "total_q"),
    (dict(max_q=0), -1, "max_seqlen_q"), (dict(max_q=-1), -1, "max_seqlen_q"), (dict(max_q=(1 << 28) + 1), -1, "max_seqlen_q"),
    (dict(total_q=1 << 30, H=2048, H_kv=2048), -1, "total_q * H"),
    (dict(q_null=True), -1, "q_strides"), (dict(o_null=True), -1, "o_strides"), (dict(l_stride=-1), -1, "l_head_stride"),
    (dict(q_strides=(-512, 64, 1)), -1, "negative"),
    # the contiguous cache: S_k is read
    (dict(S_k=0), -1, "S_k"), (dict(S_k=(1 << 28) + 1), -1, "S_k"),
    # the pool: fa2_fwd_kvcache_paged's errors, S_k ignored
    (dict(PAGED, page_size=0), -1, "page_size"), (dict(PAGED, max_blocks=0), -1, "max_blocks"), (dict(PAGED, num_blocks=0), -1, "num_blocks"),
    (dict(PAGED, max_blocks=(1 << 22) + 1), -1, "2^28"), (dict(PAGED, max_blocks=1 << 30, page_size=1 << 30), -1, "2^28"),
    (dict(PAGED, table_stride=-1), -1, "block_table_stride"),
    (dict(PAGED, variant=2, page_size=48), -2, "page_size % 64"), (dict(PAGED, variant=2, page_size=16), -2, "page_size % 64"),
    (dict(PAGED, variant=2, page_size=16, kv_dtype=_lib.FA2_DTYPE_F8E4M3), -2, "page_size % 64"),
    # descales go with an fp8 cache
    (dict(kd=0x3000, kd_strides=(2, 1)), -1, "descale"), (dict(PAGED, kd=0x3000, kd_strides=(2, 1)), -1, "descale"),
    (dict(kv_dtype=_lib.FA2_DTYPE_F8E4M3, kd=0x3000), -1, "k_descale_strides"),
    (dict(kv_dtype=_lib.FA2_DTYPE_F8E4M3, kd=0x3000, kd_strides=(-2, 1)), -1, "negative"),
    # the workspace: [num_splits][total_q * H][d + 1] floats
    (dict(num_splits=4), -1, "workspace"), (dict(num_splits=4, ws=0x2000, ws_bytes=4 * 4 * 40 * 8 * 65 - 1), -1, "workspace"),
    (dict(num_splits=0, B=1, total_q=1, max_q=1, S_k=8192), -1, "workspace"),   # auto resolves to more than 1 at this capacity
    # inherited from the fixed-N_q entry points
    (dict(ptr=None), -1, "null Q"), (dict(B=0), -1, "B must"), (dict(B=65536), -1, "B must"), (dict(H=0), -1, "H must"),
    (dict(H=8, H_kv=3), -1, "H_kv"), (dict(H_kv=0), -1, "H_kv"), (dict(num_splits=129), -1, "num_splits"),
    (dict(num_splits=-1), -1, "num_splits"), (dict(k_strides=(-1, 64, 64, 1)), -1, "negative"), (dict(window=(-2, 0)), -1, "window"),
    (dict(dtype=_lib.FA2_DTYPE_F8E4M3), -2, "fp8"), (dict(dtype=_lib.FA2_DTYPE_F8E5M2), -2, "fp8"),
    (dict(kv_dtype=_lib.FA2_DTYPE_F32), -2, "kv_dtype_enum"), (dict(kv_dtype=99), -2, "kv_dtype_enum"),
    (dict(dtype=_lib.FA2_DTYPE_F32, kv_dtype=_lib.FA2_DTYPE_F8E4M3), -2, "dtype_enum"),
    (dict(dtype=99), -2, "dtype"), (dict(d=513), -2, "[1, 512]"), (dict(d=0), -2, "[1, 512]"), (dict(variant=7), -2, "variant"),
    # a forced matrix form it cannot run
    (dict(variant=2, d=40), -2, "mfma16"), (dict(variant=2, dtype=_lib.FA2_DTYPE_F32), -2, "mfma16"),
    (dict(variant=2, H=130, H_kv=2), -2, "g = H / H_kv"), (dict(variant=2, q_strides=(8 * 64 + 4, 64, 1)), -2, "mfma16"),
])
def test_argument_errors_before_any_launch(kwargs, code, needle):
    rc, msg = _call(**kwargs)
    assert rc == code, (rc, msg)
    assert needle in msg, msg


def test_limits_pass_the_range_checks():
    """max_seqlen_q = 2^28, total_q * H = 2^40 and a capacity of 2^28 are accepted: the call gets as far as the workspace check"""
    for kw in (dict(max_q=1 << 28), dict(total_q=1 << 30, H=1024, H_kv=1024), dict(S_k=1 << 28), dict(PAGED, max_blocks=1 << 22)):
        rc, msg = _call(num_splits=2, **kw)
        assert rc == -1 and "workspace" in msg, (kw, rc, msg)


def test_workspace_formula():
    ws = _lib.kvcache_varlen_workspace_bytes
    for total_q, H, d, n in ((1, 1, 1, 2), (674, 8, 64, 3), (40, 8, 64, 4), (5000, 32, 128, 128), (7, 3, 40, 16)):
        assert ws(total_q, H, d, n) == 4 * n * total_q * H * (d + 1)       # o_part [n][total_q * H][d] then l_part, fp32
        assert ws(total_q, H, d, 1) == 0 and ws(total_q, H, d, 0) == 0
    assert ws(40, 8, 64, 500) == ws(40, 8, 64, 128)                       # FA2_KVCACHE_MAX_SPLITS
    assert ws(0, 8, 64, 4) == 0 and ws(40, 0, 64, 4) == 0
    assert ws(1 << 30, 1024, 64, 2) == 4 * 2 * (1 << 40) * 65
    assert ws((1 << 30) + 1, 1024, 64, 2) == 2 ** 63 - 1                  # beyond what a call accepts


def _unsplit(Bc, H, H_kv, total_q, max_q, d, dtype):
    """the workgroup count of the unsplit launch AUTO takes as far as the shape decides it"""
    g = H // H_kv
    mfma = dtype in (_lib.FA2_DTYPE_F16, _lib.FA2_DTYPE_BF16) and d in (64, 128) and 1 <= g <= 64 and H % H_kv == 0
    tq = tile_q(g, max_q) if mfma else 16
    return (H_kv if mfma else H) * min(Bc * -(-max_q // tq), -(-total_q // tq) + Bc)


def test_split_heuristic():
    ns = _lib.kvcache_varlen_num_splits
    bf, f32 = _lib.FA2_DTYPE_BF16, _lib.FA2_DTYPE_F32
    shapes = [(4, 32, 8, 2048, 512, 128, bf), (1, 32, 8, 2048, 2048, 128, bf), (64, 32, 8, 1087, 1024, 128, bf), (16, 32, 2, 128, 8, 128, bf),
              (1, 8, 2, 1, 1, 64, bf), (12, 8, 2, 674, 300, 64, bf), (3, 8, 2, 40, 16, 40, bf), (2, 4, 4, 7, 5, 64, f32),
              (1, 256, 2, 5, 5, 64, bf), (1, 1, 1, 1, 1, 128, bf), (200, 8, 8, 200, 1, 64, bf),
              # head counts a call refuses (H < H_kv, H % H_kv != 0): the helper answers with the VALU form's count, it does not fault
              (1, 2, 4, 5, 5, 64, bf), (2, 2, 4, 9, 5, 128, bf), (1, 1, 65535, 1, 1, 128, bf), (3, 10, 4, 40, 16, 64, bf),
              (1, 7, 2, 300, 300, 128, bf), (1, 2, 4, 5, 5, 64, f32)]
    for Bc, H, H_kv, total_q, max_q, d, dt in shapes:
        base = _unsplit(Bc, H, H_kv, total_q, max_q, d, dt)
        prev = 1
        for S_k in (1, 64, 255, 256, 512, 1000, 4096, 8192, 32768, 1 << 20, 1 << 28):
            n = ns(Bc, H, H_kv, total_q, max_q, S_k, d, dt)
            assert 1 <= n <= 128 and n >= prev, (Bc, H, H_kv, total_q, max_q, S_k, n)         # monotone in the capacity
            want = 1 if base >= 256 else max(1, min(-(-512 // base), -(-S_k // 64) // 4, 128))  # the decode rule on this count
            assert n == want, (Bc, H, H_kv, total_q, max_q, S_k, n, want, base)
            prev = n
        assert (base >= 256) == (ns(Bc, H, H_kv, total_q, max_q, 1 << 28, d, dt) == 1)
    # a uniform decode batch inside the fixed call's limit: the same count as fa2_kvcache_num_splits
    for Bc, H, H_kv, n_q in ((4, 32, 8, 1), (2, 8, 2, 5), (16, 32, 2, 2)):
        for S_k in (512, 8192, 1 << 17):
            assert ns(Bc, H, H_kv, Bc * n_q, n_q, S_k, 128, bf) == _lib.kvcache_num_splits(Bc, H, H_kv, n_q, S_k, 128, bf)
    assert ns(0, 8, 2, 4, 4, 512, 64, bf) == 1 and ns(2, 8, 2, 0, 4, 512, 64, bf) == 1 and ns(2, 8, 2, 4, 0, 512, 64, bf) == 1


def test_python_wrapper_rejects_bad_arguments():
    Q = torch.zeros(9, 8, 64, dtype=BF16)
    K = torch.zeros(2, 2, 128, 64, dtype=BF16)
    cu = torch.tensor([0, 4, 9], dtype=torch.int32)
    lens = torch.tensor([3, 50], dtype=torch.int32)
    pool = torch.zeros(10, 2, 16, 64, dtype=BF16)
    table = torch.zeros(2, 4, dtype=torch.int32)
    one = torch.ones(2, 2)
    bad = [
        dict(Q=Q[0]), dict(Q=Q[None]), dict(Q=Q[:0]),                           # rank, no rows
        dict(cu=cu.long()), dict(cu=cu.float()), dict(cu=cu[:1]), dict(cu=cu[None]), dict(cu=[0, 4, 9]),
        dict(cu=torch.zeros(6, dtype=torch.int32)[::2]), dict(cu=cu.to("meta")),
        dict(max_q=0), dict(max_q=-3), dict(max_q=(1 << 28) + 1), dict(max_q=5.0), dict(max_q=True),
        dict(cu=torch.tensor([0, 4, 6, 9], dtype=torch.int32)),                 # B = 3 against a cache and lengths of 2
        dict(K=K[0], V=K[0]), dict(V=K[:, :, :64]), dict(K=K[..., :32], V=K[..., :32]), dict(K=K[:, :, :0], V=K[:, :, :0]),
        dict(K=torch.zeros(2, 3, 128, 64, dtype=BF16)),                          # H % H_kv != 0
        dict(K=K.float(), V=K.float()), dict(Q=Q.to(torch.float8_e4m3fn)),
        dict(k_descale=one), dict(v_descale=one),                               # descales with a 16-bit cache
        dict(K=K.to(torch.float8_e4m3fn), V=K.to(torch.float8_e5m2)),
        dict(K=K.to(torch.float8_e4m3fn), V=K.to(torch.float8_e4m3fn), k_descale=torch.ones(3, 2)),
        dict(K=K.to(torch.float8_e4m3fn), V=K.to(torch.float8_e4m3fn), Q=Q.float()),
        dict(lens=lens.long()), dict(lens=lens[:1]), dict(lens=[3, 50]),
        dict(window=(1,)), dict(window=(-2, 0)), dict(window=(1.5, 0)),
        dict(num_splits=-1), dict(num_splits=129), dict(num_splits=2.0), dict(num_splits=True),
        dict(variant="mfma32"),
        dict(K=pool, V=pool, table=table.long()), dict(K=pool, V=pool, table=table[0]), dict(K=pool, V=pool, table=table[:1]),
        dict(K=pool, V=pool, table=torch.zeros(2, 8, dtype=torch.int32)[:, ::2]),
        dict(K=pool[..., :32], V=pool[..., :32], table=table),
    ]
    for kw in bad:
        k = kw.get("K", K)
        with pytest.raises(ValueError):
            fa.flash_attention_varlen_kvcache_forward(kw.get("Q", Q), k, kw.get("V", k), kw.get("cu", cu), kw.get("max_q", 5),
                                                      kw.get("lens", lens), "cpu", window=kw.get("window"),
                                                      num_splits=kw.get("num_splits", 1), variant=kw.get("variant", "auto"),
                                                      k_descale=kw.get("k_descale"), v_descale=kw.get("v_descale"),
                                                      block_table=kw.get("table"))
    # what is fine reaches the launch, which refuses CPU tensors
    k8 = K.to(torch.float8_e4m3fn)
    for kw in (dict(), dict(lens=None), dict(K=k8, V=k8, k_descale=one, v_descale=torch.tensor(2.0)), dict(K=pool, V=pool, table=table),
               dict(Q=Q.transpose(0, 1).contiguous().transpose(0, 1)), dict(window=(64, 0)), dict(max_q=1 << 28)):
        k = kw.get("K", K)
        check_varlen_kvcache_args(kw.get("Q", Q), k, kw.get("V", k), cu, kw.get("max_q", 5), kw.get("lens", lens), kw.get("window"), 1,
                                  kw.get("k_descale"), kw.get("v_descale"), kw.get("table"))
        with pytest.raises(NotImplementedError):
            fa.flash_attention_varlen_kvcache_forward(kw.get("Q", Q), k, kw.get("V", k), cu, kw.get("max_q", 5), kw.get("lens", lens), "cpu",
                                                      window=kw.get("window"), num_splits=1, k_descale=kw.get("k_descale"),
                                                      v_descale=kw.get("v_descale"), block_table=kw.get("table"))


# ----------------------------------------------------------------------------- the probe on the ragged batch
def test_ragged_helpers_are_the_probe_s():
    """per-sequence pieces are slices of the probe's own; packing and grouping are inverse; the tile of each configuration"""
    assert [tile_q(g) for g, _, _ in PROBE_CONFIGS] == [16, 8, 64, 32, 4] and tile_q(1, 5) == 5 and tile_q(64) == 1
    K, V = ragged_cache(64)
    for b, nk in enumerate(N_K):
        assert (K[b, :, nk:] == 8).all() and (V[b, :, nk:].sum(-1) == 2).all()
    g, nq = 4, 17
    Q = seq_queries(g, nq, 64, False)
    assert torch.equal(group_rows(pack_rows(Q, g, nq), g), Q)
    assert torch.equal(Q, D.probe_queries(g, nq, 64, B=3, h_kv=H_KV)[1:2])
    whole = D.decode_keep(g, nq, True, (64, 0), lens=N_K, s_k=S_K)
    for b in (1, 5, 8):
        assert torch.equal(seq_keep(g, nq, N_K[b], True, (64, 0)), whole[b:b + 1])
    assert packed_queries(g, 64, False).shape == (sum(N_Q), g * H_KV, 64)
    assert sorted(transposed_rows(g, nq).tolist()) == list(range(g * nq))           # a permutation, tile by tile
    assert torch.equal(transposed_rows(1, 40), torch.arange(40))


def _verdicts(ref, got, dtype):
    """per sequence: does (O, L) of `got` break a bar against the truth `ref`?  float32: under the one-split and the split bar"""
    out = []
    for r, t in zip(ref, got):
        if r is None:
            out.append(False)
            continue
        bars = (False, True) if dtype in (F32, F64) else (False,)
        out.append(all(bool(D.violations(t[2].to(dtype), t[3].to(dtype), r[2], r[3], dtype, split)) for split in bars))
    return out


@pytest.mark.parametrize("d", [64, 128])
def test_every_plant_breaks_a_bar_in_every_sequence_it_changes(d):
    """on the scored or on the uniform probe (the GPU file runs both), for bf16, f16 and f32 I/O"""
    changed_somewhere = {p: 0 for p in PLANTS}
    misses = []
    for g, causal, window in PROBE_CONFIGS if d == 64 else PROBE_CONFIGS[:2]:
        refs = {u: ragged_truth(g, d, causal, window, u, F32) for u in (False, True)}
        for plant in PLANTS:
            got = {u: ragged_truth(g, d, causal, window, u, F32, plant) for u in (False, True)}
            changed = [any(r is not None and not (torch.equal(r[2], t[2]) and torch.equal(r[3], t[3]))
                           for r, t in ((refs[u][b], got[u][b]) for u in (False, True))) for b in range(B)]
            changed_somewhere[plant] += sum(changed)
            for dt in (BF16, F16, F32):
                seen = [a or c for a, c in zip(_verdicts(refs[False], got[False], dt), _verdicts(refs[True], got[True], dt))]
                misses += [((g, causal, window), plant, str(dt)[6:], b, N_Q[b], N_K[b]) for b in range(B) if changed[b] and not seen[b]]
    print({p: n for p, n in changed_somewhere.items()})
    assert not misses, misses[:20]
    assert all(n > 0 for n in changed_somewhere.values()), changed_somewhere      # every plant is a real error on this batch


def test_clean_emulation_breaks_no_bar():
    """the fp32 restatement of the split kernels and the combine launch, one sequence at a time with its own n_q(b), at every
    split count"""
    bad = []
    for d, dtypes in ((64, (BF16, F16, F32)), (128, (BF16,)), (40, (F32, F64))):
        K, V = ragged_cache(d)
        for g, causal, window in PROBE_CONFIGS if d == 64 else PROBE_CONFIGS[:2]:
            for uniform in (False, True):
                for dt in dtypes:
                    ref = ragged_truth(g, d, causal, window, uniform, dt)
                    for b, r in enumerate(ref):
                        if r is None:
                            continue
                        Q, keep, O_ref, L_ref = r
                        for n, (O, L) in D.emulate_splits(Q, K[b:b + 1], V[b:b + 1], keep, [N_K[b]], D.SPLITS[1:], dt).items():
                            v = D.violations(O, L, O_ref, L_ref, dt, n > 1)
                            if v:
                                bad.append(((g, causal, window), uniform, d, str(dt)[6:], b, n, v))
    assert not bad, bad[:10]
