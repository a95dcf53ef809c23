"""The host path of KV-cache decode (csrc/fa2_decode_api.hip) as a deterministic list of calls through the raw ctypes library with
fake pointers: what tests/golden/decode_host_calls.json records and tests/test_decode_host_golden.py replays.  Not collected by
pytest.  Four kinds of case over the ten launching entry points:

  singles  a valid base call with one argument (or one group of arguments) made wrong: the code and the whole message;
  pairs    every two singles of one entry point that change different arguments, in one call: which of the two results comes
           back (0 / 1), or the whole result where it is neither: this pins the order of the checks;
  valid    calls that pass every check and steer the dispatch.  A process that sees no device gets FA2_ERR_LAUNCH from the first
           launch attempted, whose message names it: the text is kept up to "launch failed" (a forced form that cannot run is -2);
  helpers  the three split heuristics and the two workspace sizes over a grid: the integers.

    python tests/decode_host_cases.py --record     writes the fixture from the library in the tree (and prints the
                                                   fa2_set_error sites of fa2_decode_api.hip no single reached)
    python tests/decode_host_cases.py --replay     prints one JSON line: {"skipped": ...} or {"mismatches": [...], "counts": ...}

Both refuse to make a library call while a device is visible (start them with HIP_VISIBLE_DEVICES=-1): a call that passes the
checks would otherwise launch on a fake pointer."""
import ctypes
import hashlib
import itertools
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "decode_host_calls.json")
SOURCE = os.path.join(ROOT, "flash_attention_dlrs_amd", "csrc", "fa2_decode_api.hip")

F32, F16, BF16, F8E5, F8E4, F64 = range(6)  # FA2_DTYPE_*
NAN = float("nan")
P = 0x1000  # the fake pointer of every tensor unless a case says otherwise


def contiguous(*shape):
    out, s = [], 1
    for n in reversed(shape):
        out.append(s)
        s *= n
    return tuple(reversed(out))


def join(*dicts, **more):
    out = {}
    for d in dicts + (more,):
        out.update(d)
    return out


# Every entry point: its parameters in the header's order, and a base call that passes every check (B 2, H 8, H_kv 2, d 64, bf16,
# num_splits 1).  A case is a dict of replacements.
_ATT4 = "Q K V O L q_strides k_strides v_strides o_strides l_strides cache_seqlens"
_ATT3 = "Q K V O L q_strides k_strides v_strides o_strides l_head_stride cu_seqlens_q cache_seqlens"
_TAIL = "causal scale window_left window_right num_splits workspace workspace_bytes"
_DESC = "k_descale v_descale k_descale_strides v_descale_strides"
_ROT = "rotary_cos rotary_sin rotary_cos_stride rotary_sin_stride S_rot rotary_dim rotary_interleaved"
_POOL = "num_blocks page_size max_blocks"
ORDER = {
    "fa2_fwd_kvcache": f"{_ATT4} B H H_kv N_q S_k d dtype_enum {_TAIL} hip_stream",
    "fa2_fwd_kvcache_variant": f"{_ATT4} B H H_kv N_q S_k d dtype_enum {_TAIL} hip_stream variant",
    "fa2_fwd_kvcache_fp8": f"{_ATT4} {_DESC} B H H_kv N_q S_k d dtype_enum kv_dtype_enum {_TAIL} variant hip_stream",
    "fa2_fwd_kvcache_paged": f"{_ATT4} block_table block_table_stride {_DESC} B H H_kv N_q {_POOL} d dtype_enum kv_dtype_enum {_TAIL} "
                             f"variant hip_stream",
    "fa2_fwd_kvcache_mla": f"{_ATT4} block_table block_table_stride B H H_kv N_q {_POOL} d d_v dtype_enum {_TAIL} variant hip_stream",
    "fa2_fwd_kvcache_varlen": f"{_ATT3} block_table block_table_stride {_DESC} B H H_kv total_q max_seqlen_q S_k {_POOL} d dtype_enum "
                              f"kv_dtype_enum {_TAIL} variant hip_stream",
    "fa2_kvcache_append": f"K V k_strides v_strides block_table block_table_stride k_new v_new k_new_strides v_new_strides cache_seqlens "
                          f"seqlens_out {_DESC} {_ROT} Q q_rot q_strides H N_q q_pos_per_row B H_kv N_new S_k {_POOL} d dtype_enum "
                          f"kv_dtype_enum hip_stream",
    "fa2_fwd_kvcache_append": f"{_ATT4} seqlens_out block_table block_table_stride {_DESC} k_new v_new k_new_strides v_new_strides {_ROT} "
                              f"q_rot B H H_kv N_q N_new S_k {_POOL} d dtype_enum kv_dtype_enum {_TAIL} variant hip_stream",
    "fa2_kvcache_append_varlen": f"K V k_strides v_strides block_table block_table_stride k_new v_new k_new_strides v_new_strides "
                                 f"cu_seqlens_new cache_seqlens seqlens_out {_DESC} {_ROT} Q q_rot q_strides H q_pos_per_row B H_kv "
                                 f"total_new max_seqlen_new S_k {_POOL} d dtype_enum kv_dtype_enum hip_stream",
    "fa2_fwd_kvcache_varlen_append": f"{_ATT3} seqlens_out block_table block_table_stride {_DESC} k_new v_new k_new_strides v_new_strides "
                                     f"{_ROT} q_rot B H H_kv total_q max_seqlen_q S_k {_POOL} d dtype_enum kv_dtype_enum {_TAIL} variant "
                                     f"hip_stream",
}
ORDER = {k: v.split() for k, v in ORDER.items()}
ENTRY_POINTS = tuple(ORDER)

_COMMON = dict(Q=P, K=P, V=P, O=P, L=P, cache_seqlens=None, B=2, H=8, H_kv=2, d=64, dtype_enum=BF16, causal=0, scale=1.0, window_left=-1,
               window_right=-1, num_splits=1, workspace=None, workspace_bytes=0, hip_stream=None, variant=0)
_FIXED = join(_COMMON, q_strides=contiguous(2, 8, 1, 64), k_strides=contiguous(2, 2, 512, 64), v_strides=contiguous(2, 2, 512, 64),
              o_strides=contiguous(2, 8, 1, 64), l_strides=(8, 1), N_q=1, S_k=512)
_NO_DESC = dict(k_descale=None, v_descale=None, k_descale_strides=None, v_descale_strides=None)
_NO_TABLE = dict(block_table=None, block_table_stride=0, num_blocks=32, page_size=64, max_blocks=8)
_PACKED = join(_COMMON, _NO_DESC, _NO_TABLE, q_strides=contiguous(40, 8, 64), k_strides=contiguous(2, 2, 512, 64),
               v_strides=contiguous(2, 2, 512, 64), o_strides=contiguous(40, 8, 64), l_head_stride=40, cu_seqlens_q=0x5000, total_q=40,
               max_seqlen_q=32, S_k=512, kv_dtype_enum=BF16)
_NO_ROT = dict(rotary_cos=None, rotary_sin=None, rotary_cos_stride=32, rotary_sin_stride=32, S_rot=512, rotary_dim=64, rotary_interleaved=0)
_NEW = dict(k_new=0x2000, v_new=0x2000, cache_seqlens=0x3000, seqlens_out=0x3100, q_rot=0x6000, kv_dtype_enum=BF16)
BASE = {
    "fa2_fwd_kvcache": _FIXED,
    "fa2_fwd_kvcache_variant": _FIXED,
    "fa2_fwd_kvcache_fp8": join(_FIXED, _NO_DESC, kv_dtype_enum=F8E4),
    "fa2_fwd_kvcache_paged": join(_FIXED, _NO_DESC, _NO_TABLE, block_table=0x4000, block_table_stride=8, kv_dtype_enum=BF16,
                                  k_strides=contiguous(32, 2, 64, 64), v_strides=contiguous(32, 2, 64, 64)),
    # contiguous: page_size carries S_k; V aliases K
    "fa2_fwd_kvcache_mla": join(_FIXED, _NO_TABLE, H=16, H_kv=1, d=576, d_v=512, page_size=512, q_strides=contiguous(2, 16, 1, 576),
                                k_strides=contiguous(2, 1, 512, 576), v_strides=contiguous(2, 1, 512, 576),
                                o_strides=contiguous(2, 16, 1, 512), l_strides=(16, 1)),
    "fa2_fwd_kvcache_varlen": _PACKED,
    "fa2_kvcache_append": join(_COMMON, _NO_DESC, _NO_TABLE, _NO_ROT, _NEW, Q=0x5000, k_strides=contiguous(2, 2, 256, 64),
                               v_strides=contiguous(2, 2, 256, 64), k_new_strides=contiguous(2, 2, 1, 64),
                               v_new_strides=contiguous(2, 2, 1, 64), q_strides=contiguous(2, 8, 1, 64), N_q=1, N_new=1, S_k=256,
                               q_pos_per_row=0),
    "fa2_fwd_kvcache_append": join(_FIXED, _NO_DESC, _NO_TABLE, _NO_ROT, _NEW, Q=0x5000, k_strides=contiguous(2, 2, 256, 64),
                                   v_strides=contiguous(2, 2, 256, 64), k_new_strides=contiguous(2, 2, 1, 64),
                                   v_new_strides=contiguous(2, 2, 1, 64), N_new=1, S_k=256),
    "fa2_kvcache_append_varlen": join(_COMMON, _NO_DESC, _NO_TABLE, _NO_ROT, _NEW, Q=0x5000, k_strides=contiguous(2, 2, 256, 64),
                                      v_strides=contiguous(2, 2, 256, 64), k_new_strides=contiguous(5, 2, 64),
                                      v_new_strides=contiguous(5, 2, 64), q_strides=contiguous(5, 8, 64), cu_seqlens_new=0x2800,
                                      total_new=5, max_seqlen_new=3, S_k=256, q_pos_per_row=0),
    "fa2_fwd_kvcache_varlen_append": join(_PACKED, _NO_ROT, _NEW, Q=0x5000, cu_seqlens_q=0x2800, k_strides=contiguous(2, 2, 256, 64),
                                          v_strides=contiguous(2, 2, 256, 64), q_strides=contiguous(5, 8, 64), o_strides=contiguous(5, 8, 64),
                                          l_head_stride=5, k_new_strides=contiguous(5, 2, 64), v_new_strides=contiguous(5, 2, 64),
                                          total_q=5, max_seqlen_q=3, S_k=256),
}

TABLE = dict(block_table=0x4000, block_table_stride=8)
ROT = dict(rotary_cos=0x7000, rotary_sin=0x7100)
BIG = dict(workspace=0x2000, workspace_bytes=1 << 40)


def _attention_singles(name):
    """What goes wrong in the attention's arguments (check_decode), for the entry points that have them."""
    b = {k: v for k, v in BASE[name].items() if k in ORDER[name]}
    fixed, packed, mla, fused = "N_q" in b and "total_q" not in b, "total_q" in b, name.endswith("_mla"), "seqlens_out" in b
    s = [dict(O=None), dict(L=None), dict(k_strides=None), dict(v_strides=None), dict(o_strides=None),
         dict(B=0), dict(B=65536), dict(H=0), dict(H=65536, H_kv=1), dict(H_kv=0), dict(H=8, H_kv=3),
         dict(window_left=-2), dict(window_right=-2), dict(k_strides=(-1, 64, 64, 1)), dict(v_strides=(64, 64, -64, 1)),
         dict(scale=NAN), dict(num_splits=-1), dict(num_splits=129), dict(num_splits=4), dict(num_splits=4, workspace=0x2000, workspace_bytes=16),
         dict(dtype_enum=99), dict(dtype_enum=F8E4), dict(dtype_enum=F8E5), dict(variant=7), dict(variant=-1)]
    if "kv_dtype_enum" in b:  # (f64 is a dtype of the entry points without one)
        s += [dict(dtype_enum=F64)]
    if not fused:  # (the fused calls' Q, K, V, q_strides and d are the append's to refuse)
        s += [dict(Q=None), dict(K=None), dict(V=None), dict(q_strides=None), dict(d=0)]
    s += [dict(d=577), dict(d_v=0), dict(d_v=513), dict(variant=2)] if mla else [dict(d=513), dict(variant=3)]
    if fixed:
        s += [dict(l_strides=None), dict(l_strides=(8, -1)), dict(q_strides=(512, 64, -64, 1)), dict(o_strides=(512, 64, 64, -1)),
              dict(B=65535, H=65535, H_kv=1, N_q=1 << 28, **BIG)]
        if not fused:
            s += [dict(N_q=0), dict(N_q=(1 << 28) + 1)]
    if packed:
        s += [dict(l_head_stride=-1), dict(o_strides=(512, -64, 1)), dict(total_q=1 << 28, H=8192, H_kv=8192)]
        if not fused:
            s += [dict(cu_seqlens_q=None), dict(total_q=0), dict(total_q=-5), dict(max_seqlen_q=0), dict(max_seqlen_q=(1 << 28) + 1),
                  dict(q_strides=(-512, 64, 1)), dict(total_q=1 << 30, H=2048, H_kv=2048)]
    if "S_k" in b and not fused:
        s += [dict(S_k=0), dict(S_k=(1 << 28) + 1)]
    if mla:
        s += [dict(page_size=0), dict(page_size=(1 << 28) + 1)]
    if "block_table" in b and not fused:
        s += [dict(TABLE, page_size=0), dict(TABLE, max_blocks=0), dict(TABLE, num_blocks=-1), dict(TABLE, max_blocks=(1 << 22) + 1),
              dict(TABLE, max_blocks=1 << 30, page_size=1 << 30), dict(TABLE, block_table_stride=-1)]
    if name.endswith("_paged"):
        s += [dict(block_table=None)]
    if "k_descale" in b and not fused:
        if b["kv_dtype_enum"] == BF16:
            s += [dict(k_descale=0x3000, k_descale_strides=(2, 1)), dict(v_descale=0x3000, v_descale_strides=(2, 1))]
        fp8 = {} if b["kv_dtype_enum"] != BF16 else dict(kv_dtype_enum=F8E4)
        s += [dict(fp8, k_descale=0x3000), dict(fp8, v_descale=0x3000), dict(fp8, k_descale=0x3000, k_descale_strides=(-2, 1)),
              dict(fp8, v_descale=0x3000, v_descale_strides=(0, -1)), dict(kv_dtype_enum=F32), dict(kv_dtype_enum=99),
              dict(fp8, dtype_enum=F32), dict(dtype_enum=F8E4, kv_dtype_enum=F8E5)]
        if fp8 == {}:
            s += [dict(kv_dtype_enum=BF16), dict(kv_dtype_enum=F16)]
    # a forced form that cannot run
    if mla:
        s += [dict(variant=3, d=128, d_v=64), dict(variant=3, d_v=256), dict(variant=3, V=0x9000), dict(variant=3, dtype_enum=F32),
              dict(variant=3, scale=0.0), dict(variant=3, k_strides=(512 * 1152, 512 * 1152, 1152, 2)), dict(variant=3, Q=0x1004),
              dict(variant=3, **TABLE, page_size=48)]
    elif name != "fa2_fwd_kvcache":
        if b.get("kv_dtype_enum", BF16) == BF16:
            s += [dict(variant=2, dtype_enum=F32, kv_dtype_enum=F32) if "kv_dtype_enum" in b else dict(variant=2, dtype_enum=F32)]
        s += [dict(variant=2, Q=0x1004), dict(variant=2, k_strides=(2 * 512 * 128, 512 * 128, 128, 2))]
        s += [dict(variant=2, H=130, H_kv=2)] if packed else [dict(variant=2, H=40, H_kv=1, N_q=2)]
        if not fused:
            s += [dict(variant=2, d=40)]
        if "block_table" in b:
            s += [dict(variant=2, **TABLE, page_size=48)]
    if name == "fa2_fwd_kvcache":  # it has no variant argument
        s = [c for c in s if "variant" not in c]
    return s


def _append_singles(name):
    """What goes wrong in the append's arguments (check_append)."""
    b = {k: v for k, v in BASE[name].items() if k in ORDER[name]}
    packed, fused = "N_new" not in b, "O" in ORDER[name]
    s = [dict(K=None), dict(V=None), dict(k_strides=None), dict(v_strides=None), dict(k_new=None), dict(v_new=None),
         dict(k_new_strides=None), dict(v_new_strides=None), dict(cache_seqlens=None), dict(seqlens_out=None), dict(seqlens_out=0x3000),
         dict(TABLE, page_size=0), dict(TABLE, max_blocks=0), dict(TABLE, num_blocks=0), dict(TABLE, max_blocks=(1 << 22) + 1),
         dict(TABLE, max_blocks=1 << 30, page_size=1 << 30), dict(TABLE, block_table_stride=-1), dict(S_k=0), dict(S_k=(1 << 28) + 1),
         dict(B=0), dict(B=65536), dict(H_kv=0), dict(H_kv=65536), dict(H=8, H_kv=3), dict(H=0), dict(H=65536), dict(q_strides=None),
         dict(k_strides=(-1, 64, 64, 1)), dict(v_strides=(64, 64, 64, -1)),
         dict(k_descale=0x3000, k_descale_strides=(2, 1)), dict(v_descale=0x3000), dict(dtype_enum=F8E4), dict(dtype_enum=F8E5),
         dict(dtype_enum=F8E4, kv_dtype_enum=F8E4), dict(dtype_enum=F8E5, kv_dtype_enum=F8E5),
         dict(kv_dtype_enum=F8E4, k_descale=0x3000), dict(kv_dtype_enum=F8E4, v_descale=0x3000),
         dict(kv_dtype_enum=F8E4, k_descale=0x3000, k_descale_strides=(-2, 1)), dict(kv_dtype_enum=F8E5, v_descale=0x3000, v_descale_strides=(0, -1)),
         dict(kv_dtype_enum=F32), dict(kv_dtype_enum=99), dict(dtype_enum=F32, kv_dtype_enum=F8E4), dict(dtype_enum=F8E4, kv_dtype_enum=F8E5),
         dict(dtype_enum=99), dict(d=0), dict(d=513),
         dict(rotary_cos=0x7000), dict(rotary_sin=0x7100), dict(ROT, rotary_dim=63), dict(ROT, rotary_dim=0), dict(ROT, rotary_dim=66),
         dict(ROT, S_rot=0), dict(ROT, rotary_cos_stride=-32), dict(ROT, rotary_sin_stride=-1), dict(ROT, q_rot=None)]
    if packed:
        new = ("cu_seqlens_q", "total_q", "max_seqlen_q") if fused else ("cu_seqlens_new", "total_new", "max_seqlen_new")
        s += [{new[0]: None}, {new[1]: 0}, {new[1]: -1}, {new[1]: (1 << 28) + 1}, {new[2]: 0}, {new[2]: -4}, {new[2]: (1 << 28) + 1},
              {new[1]: 1 << 28, "H_kv": 4096, "H": 8192}, dict(ROT, **{new[1]: 1 << 28, "H_kv": 1, "H": 8192}),
              dict(k_new_strides=(64, -64, 1)), dict(v_new_strides=(-1, 64, 1)), dict(q_strides=(64, 64, -1))]
    else:
        s += [dict(N_new=0), dict(N_new=-1), dict(N_new=(1 << 28) + 1), dict(N_q=0), dict(N_q=(1 << 28) + 1),
              dict(k_new_strides=(64, 64, -64, 1)), dict(v_new_strides=(-1, 64, 64, 1)), dict(q_strides=(64, 64, 64, -1))]
    if fused:  # the append reads Q only beside rotary tables: a null one is the attention's to refuse
        s += [dict(Q=None), dict(ROT, Q=None)]
    return s


def singles(name):
    s = []
    if "k_new" in BASE[name]:
        s += _append_singles(name)
    if "O" in ORDER[name]:
        s += _attention_singles(name)
    s = [c for k, c in enumerate(s) if c not in s[:k]]  # (the fused calls: what both lists name)
    for c in s:
        assert set(c) <= set(ORDER[name]), (name, c)
    return s


def pairs(name):
    """(i, j, the two singles in one call) for every two singles of `name` that change different arguments."""
    s = singles(name)
    return [(i, j, dict(s[i], **s[j])) for i, j in itertools.combinations(range(len(s)), 2) if not set(s[i]) & set(s[j])]


def _shape(H=8, H_kv=2, N_q=1, S_k=512, d=64, B=2):
    """The fixed call at another shape, contiguous."""
    return dict(B=B, H=H, H_kv=H_kv, N_q=N_q, S_k=S_k, d=d, q_strides=contiguous(B, H, N_q, d), o_strides=contiguous(B, H, N_q, d),
                k_strides=contiguous(B, H_kv, S_k, d), v_strides=contiguous(B, H_kv, S_k, d), l_strides=(H * N_q, N_q))


def _packed_shape(H, H_kv, total=40, d=64):
    return dict(H=H, H_kv=H_kv, q_strides=contiguous(total, H, d), o_strides=contiguous(total, H, d))


def valid():
    """(entry point, replacements): calls that pass every check, chosen to steer the dispatch."""
    v = "fa2_fwd_kvcache_variant"
    ws16, ws8 = dict(workspace=0x2000, workspace_bytes=1 << 30), dict(workspace=0x2008, workspace_bytes=1 << 30)
    out = [("fa2_fwd_kvcache", {}), (v, {}), (v, dict(dtype_enum=F16)), (v, dict(dtype_enum=F32)), (v, dict(dtype_enum=F64)),
           (v, _shape(d=128)), (v, _shape(d=40)), (v, _shape(H=64, H_kv=1)), (v, _shape(H=65, H_kv=1)), (v, _shape(H=16, H_kv=1, N_q=4)),
           (v, _shape(H=13, H_kv=1, N_q=5)), (v, _shape(N_q=17)),
           (v, dict(Q=0x1008)), (v, dict(K=0x1008)), (v, dict(O=0x1008)), (v, dict(k_strides=(2 * 512 * 128, 512 * 128, 128, 2))),
           (v, dict(q_strides=(1024, 128, 128, 2))), (v, dict(scale=0.0)), (v, dict(scale=-1.0)), (v, dict(causal=1)),
           (v, dict(window_left=4, window_right=0)), (v, dict(cache_seqlens=0x3000))]
    for n in (1, 4):
        for ws in (ws16, ws8):
            out += [(v, dict(ws, num_splits=n)), (v, dict(ws, num_splits=n, variant=1)), (v, dict(ws, num_splits=n, variant=2)),
                    ("fa2_fwd_kvcache_varlen", dict(ws, num_splits=n)), ("fa2_fwd_kvcache_mla", dict(ws, num_splits=n))]
    out += [(v, dict(_shape(S_k=8192, B=1), **ws16, num_splits=0))]
    for variant in (0, 1, 2):
        out += [(v, dict(variant=variant)), (v, dict(_shape(d=40), variant=variant)), (v, dict(dtype_enum=F32, variant=variant)),
                ("fa2_fwd_kvcache_fp8", dict(variant=variant)), ("fa2_fwd_kvcache_fp8", dict(variant=variant, kv_dtype_enum=F8E5)),
                ("fa2_fwd_kvcache_fp8", dict(variant=variant, k_descale=0x3000, k_descale_strides=(2, 1), v_descale=0x3100,
                                             v_descale_strides=(0, 0))),
                ("fa2_fwd_kvcache_fp8", dict(variant=variant, k_strides=(2 * 512 * 72, 512 * 72, 72, 1))),
                ("fa2_fwd_kvcache_paged", dict(variant=variant)), ("fa2_fwd_kvcache_paged", dict(variant=variant, page_size=48)),
                ("fa2_fwd_kvcache_paged", dict(variant=variant, kv_dtype_enum=F8E4)),
                ("fa2_fwd_kvcache_paged", dict(variant=variant, kv_dtype_enum=F8E4, page_size=48)),
                ("fa2_fwd_kvcache_varlen", dict(variant=variant)), ("fa2_fwd_kvcache_varlen", dict(_packed_shape(64, 1), variant=variant)),
                ("fa2_fwd_kvcache_varlen", dict(_packed_shape(65, 1), variant=variant)),
                ("fa2_fwd_kvcache_varlen", dict(variant=variant, dtype_enum=F32, kv_dtype_enum=F32)),
                ("fa2_fwd_kvcache_varlen", dict(variant=variant, **TABLE)),
                ("fa2_fwd_kvcache_varlen", dict(variant=variant, **TABLE, page_size=48)),
                ("fa2_fwd_kvcache_varlen", dict(variant=variant, kv_dtype_enum=F8E4, k_descale=0x3000, k_descale_strides=(2, 1))),
                ("fa2_fwd_kvcache_varlen", dict(variant=variant, Q=0x1008))]
    for variant in (0, 1, 3):
        out += [("fa2_fwd_kvcache_mla", dict(variant=variant)), ("fa2_fwd_kvcache_mla", dict(variant=variant, V=0x9000)),
                ("fa2_fwd_kvcache_mla", dict(variant=variant, d_v=256, o_strides=contiguous(2, 16, 1, 256))),
                ("fa2_fwd_kvcache_mla", dict(variant=variant, d=128, d_v=64)),
                ("fa2_fwd_kvcache_mla", dict(variant=variant, **TABLE, page_size=64)),
                ("fa2_fwd_kvcache_mla", dict(variant=variant, **TABLE, page_size=48)),
                ("fa2_fwd_kvcache_mla", dict(variant=variant, K=0x1008, V=0x1008)), ("fa2_fwd_kvcache_mla", dict(variant=variant, scale=0.0)),
                ("fa2_fwd_kvcache_mla", dict(variant=variant, H=128, q_strides=contiguous(2, 128, 1, 576),
                                             o_strides=contiguous(2, 128, 1, 512), l_strides=(128, 1)))]
    for name in ("fa2_kvcache_append", "fa2_kvcache_append_varlen"):
        out += [(name, {}), (name, ROT), (name, dict(Q=None, q_rot=None, q_strides=None, H=0)), (name, TABLE),
                (name, dict(kv_dtype_enum=F8E4, k_descale=0x3000, k_descale_strides=(2, 1))), (name, dict(ROT, rotary_interleaved=1))]
    for name in ("fa2_fwd_kvcache_append", "fa2_fwd_kvcache_varlen_append"):
        for variant in (0, 1, 2):
            out += [(name, dict(variant=variant)), (name, dict(ROT, variant=variant)), (name, dict(ROT, variant=variant, causal=1)),
                    (name, dict(TABLE, variant=variant)), (name, dict(TABLE, variant=variant, page_size=48)),
                    (name, dict(ROT, variant=variant, dtype_enum=F32, kv_dtype_enum=F32)),
                    (name, dict(variant=variant, kv_dtype_enum=F8E4)), (name, dict(variant=variant, O=0x1008))]
    for name, c in out:
        assert set(c) <= set(ORDER[name]), (name, c)
    return out


def helpers():
    """(function, argument tuples): the grid of the split heuristics and the workspace sizes."""
    caps = sorted({-1, 0, 1, 63, 64, 255, 256, 257, 4096, 1 << 28} | {64 * 4 * n + e for n in (1, 2, 3, 16, 127, 128) for e in (-1, 0, 1)})
    dts = (BF16, F16, F32, F8E4, 99)
    # (B, H, H_kv, N_q, d, dtype): both sides of fa2_decode_mfma16_shape, bases of 255 / 256 / 257 in either form
    fixed = [(1, 32, 8, 1, 128, dt) for dt in dts] + [(1, 32, 8, 1, d, BF16) for d in (64, 40, 0, 576)] + \
            [(1, 64, 1, 1, 128, BF16), (1, 65, 1, 1, 128, BF16), (1, 16, 1, 4, 64, BF16), (1, 13, 1, 5, 64, BF16), (2, 8, 2, 16, 64, F32),
             (2, 8, 2, 17, 64, F32), (1, 7, 2, 1, 64, BF16), (1, 2, 4, 1, 64, BF16), (1, 130, 2, 1, 64, BF16),
             (255, 8, 1, 1, 64, BF16), (256, 8, 1, 1, 64, BF16), (257, 8, 1, 1, 64, BF16), (85, 3, 3, 1, 64, BF16), (51, 5, 1, 1, 64, F32),
             (255, 1, 1, 1, 64, F32), (256, 1, 1, 16, 64, F32), (257, 1, 1, 1, 64, F32), (128, 1, 1, 17, 64, F32), (3, 32, 4, 1, 128, F16),
             (0, 8, 2, 1, 64, BF16), (2, 0, 2, 1, 64, BF16), (2, 8, 0, 1, 64, BF16), (2, 8, 2, 0, 64, BF16), (-1, 8, 2, 1, 64, BF16),
             (2, 8, -2, 1, 64, BF16), (65535, 65535, 1, 1, 64, BF16), (1, 1, 1, 1 << 28, 64, F32)]
    out = [("fa2_kvcache_num_splits", [(B, H, H_kv, N_q, S_k, d, dt) for B, H, H_kv, N_q, d, dt in fixed for S_k in caps])]
    # (B, H, H_kv, total_q, max_q, d, dtype): both sides of fa2_decode_mfma16_v_shape, either bound of the tile count
    packed = [(4, 32, 8, 2048, 512, 128, BF16), (1, 32, 8, 2048, 2048, 128, F16), (64, 32, 8, 1087, 1024, 128, BF16), (16, 32, 2, 128, 8, 128, BF16),
              (1, 8, 2, 1, 1, 64, BF16), (12, 8, 2, 674, 300, 64, BF16), (3, 8, 2, 40, 16, 40, BF16), (2, 4, 4, 7, 5, 64, F32),
              (1, 256, 2, 5, 5, 64, BF16), (1, 64, 1, 5, 5, 64, BF16), (1, 65, 1, 5, 5, 64, BF16), (1, 2, 4, 5, 5, 64, BF16),
              (3, 10, 4, 40, 16, 64, BF16), (1, 7, 2, 300, 300, 128, BF16), (1, 1, 65535, 1, 1, 128, BF16), (200, 8, 8, 200, 1, 64, BF16),
              (255, 1, 1, 255, 1, 64, BF16), (256, 1, 1, 256, 1, 64, BF16), (257, 1, 1, 257, 1, 64, BF16), (1, 1, 1, 254 * 64, 254 * 64, 64, BF16),
              (1, 1, 1, 255 * 64, 255 * 64, 64, BF16), (1, 1, 1, 256 * 64, 256 * 64, 64, BF16), (1, 255, 255, 1, 1, 64, F32),
              (1, 257, 257, 1, 1, 64, F32), (1, 16, 1, 255 * 16, 255 * 16, 64, F32), (5, 51, 51, 5, 1, 40, F16),
              (0, 8, 2, 4, 4, 64, BF16), (2, 8, 2, 0, 4, 64, BF16), (2, 8, 2, 4, 0, 64, BF16), (2, 0, 2, 4, 4, 64, BF16), (2, 8, 0, 4, 4, 64, BF16),
              (2, 8, -1, 4, 4, 64, BF16), (2, 8, 2, 4, 4, 64, 99)]
    out += [("fa2_kvcache_varlen_num_splits", [(B, H, H_kv, t, m, S_k, d, dt) for B, H, H_kv, t, m, d, dt in packed for S_k in caps])]
    # (B, H, H_kv, N_q, d, d_v, dtype): both sides of fa2_decode_mla16_shape, bases of 255 / 256 / 257 row tiles
    mla = [(1, 128, 1, 1, 576, 512, BF16), (1, 128, 1, 1, 576, 512, F16), (1, 128, 1, 1, 576, 512, F32), (1, 128, 1, 1, 576, 256, BF16),
           (1, 128, 1, 1, 128, 64, BF16), (1, 128, 1, 1, 64, 64, BF16), (4, 16, 1, 1, 576, 512, BF16), (4, 16, 1, 4, 576, 512, BF16),
           (4, 16, 1, 5, 576, 512, BF16), (1, 65, 1, 1, 576, 512, BF16), (1, 7, 2, 1, 576, 512, BF16), (1, 2, 4, 1, 576, 512, BF16),
           (255, 16, 1, 1, 576, 512, BF16), (256, 16, 1, 1, 576, 512, BF16), (257, 16, 1, 1, 576, 512, BF16), (85, 3, 3, 1, 576, 512, BF16),
           (64, 128, 1, 2, 576, 512, BF16), (127, 65, 1, 1, 576, 512, BF16), (128, 65, 1, 1, 576, 512, BF16), (16, 16, 1, 1, 576, 512, F32),
           (0, 16, 1, 1, 576, 512, BF16), (2, 0, 1, 1, 576, 512, BF16), (2, 16, 0, 1, 576, 512, BF16), (2, 16, 1, 0, 576, 512, BF16),
           (2, 16, -1, 1, 576, 512, BF16)]
    out += [("fa2_kvcache_mla_num_splits", [(B, H, H_kv, N_q, S_k, d, d_v, dt) for B, H, H_kv, N_q, d, d_v, dt in mla for S_k in caps])]
    splits = (-1, 0, 1, 2, 3, 128, 129, 500)
    rows = [(1, 32, 1), (4, 8, 5), (3, 6, 2), (0, 8, 1), (2, 0, 1), (2, 8, 0), (-1, 8, 1), (65535, 8, 1), (65536, 8, 1), (2, 65535, 1), (2, 65536, 1),
            (2, 8, 1 << 28), (2, 8, (1 << 28) + 1), (1 << 14, 1 << 14, 1 << 12), (1 << 14, 1 << 14, (1 << 12) + 1), (65535, 65535, 256),
            (65535, 65535, 257), (65535, 65535, 1 << 28)]
    out += [("fa2_kvcache_workspace_bytes", [(B, H, N_q, d, n) for B, H, N_q in rows for d in (-1, 0, 1, 40, 64, 512, 513, 576) for n in splits])]
    packed_rows = [(1, 1), (674, 8), (40, 8), (0, 8), (40, 0), (-3, 8), (40, -1), (40, 65535), (40, 65536), (1 << 30, 1024), ((1 << 30) + 1, 1024),
                   ((1 << 31) - 1, 65535)]
    out += [("fa2_kvcache_varlen_workspace_bytes", [(t, H, d, n) for t, H in packed_rows for d in (-1, 0, 1, 40, 64, 512, 513) for n in splits])]
    return out


def _array(v):
    return None if v is None else (ctypes.c_int64 * len(v))(*v)


def call(lib, name, case):
    """(code, message) of entry point `name` at its base call with `case`'s replacements.  The message of a launch failure ends at
    "launch failed": what follows is the runtime's wording."""
    a = dict(BASE[name], **case)
    rc = getattr(lib, name)(*[_array(a[p]) if p.endswith("_strides") else a[p] for p in ORDER[name]])
    msg = lib.fa2_last_error().decode()
    cut = msg.find("launch failed")
    return [rc, msg if cut < 0 else msg[:cut + len("launch failed")]]


def digest():
    """Of the case lists: a fixture recorded from another generator is refused instead of compared case by case."""
    text = repr([(n, singles(n)) for n in ENTRY_POINTS]) + repr(valid()) + repr(helpers())
    return hashlib.sha256(text.encode()).hexdigest()[:16]


def run(lib):
    """Every case against `lib`, in the fixture's form.  Messages are stored once, in "messages"; a result is [code, index]."""
    messages = {}
    ref = lambda r: [r[0], messages.setdefault(r[1], len(messages))]
    out = {"digest": digest(), "singles": {}, "pairs": {}, "valid": [], "helpers": {}}
    for name in ENTRY_POINTS:
        got = [call(lib, name, c) for c in singles(name)]
        out["singles"][name] = [ref(r) for r in got]
        which, other = [], {}
        for k, (i, j, c) in enumerate(pairs(name)):
            r = call(lib, name, c)
            which.append("0" if r == got[i] else "1" if r == got[j] else "2")
            if which[-1] == "2":
                other[str(k)] = ref(r)
        out["pairs"][name] = {"which": "".join(which), "other": other}
    out["valid"] = [ref(call(lib, name, c)) for name, c in valid()]
    for name, grid in helpers():
        out["helpers"][name] = [int(getattr(lib, name)(*args)) for args in grid]
    out["messages"] = list(messages)
    return out


def mismatches(want, got):
    """Human-readable differences of two run() results, each case named."""
    if want["digest"] != got["digest"]:
        return [f"the fixture was recorded from another case list (digest {want['digest']}, now {got['digest']}): record it again "
                f"from a build of the parent"]
    text = lambda run_, r: (r[0], run_["messages"][r[1]])
    bad = []
    for name in ENTRY_POINTS:
        s = singles(name)
        for c, w, g in zip(s, want["singles"][name], got["singles"][name]):
            if text(want, w) != text(got, g):
                bad.append(f"single {name} {c}: want {text(want, w)}, got {text(got, g)}")
        wp, gp = want["pairs"][name], got["pairs"][name]
        for k, (i, j, c) in enumerate(pairs(name)):
            w = wp["which"][k] if wp["which"][k] != "2" else text(want, wp["other"][str(k)])
            g = gp["which"][k] if gp["which"][k] != "2" else text(got, gp["other"][str(k)])
            if w != g:
                bad.append(f"pair {name} {s[i]} + {s[j]}: want {w}, got {g} (0 / 1: the first / second single's result)")
    for (name, c), w, g in zip(valid(), want["valid"], got["valid"]):
        if text(want, w) != text(got, g):
            bad.append(f"valid {name} {c}: want {text(want, w)}, got {text(got, g)}")
    for name, grid in helpers():
        for args, w, g in zip(grid, want["helpers"][name], got["helpers"][name]):
            if w != g:
                bad.append(f"helper {name}{args}: want {w}, got {g}")
    return bad


def counts(fixture):
    return {"singles": {n: len(v) for n, v in fixture["singles"].items()}, "pairs": {n: len(v["which"]) for n, v in fixture["pairs"].items()},
            "valid": {n: sum(1 for m, _ in valid() if m == n) for n in ENTRY_POINTS}, "valid_stored": len(fixture["valid"]),
            "helpers": {n: len(v) for n, v in fixture["helpers"].items()}}


def error_sites():
    """The format strings of every fa2_set_error call of fa2_decode_api.hip, and the two of fa2_check_gqa, as regular expressions."""
    src = open(SOURCE).read()
    formats = ["H_kv must be >= 1 (got H_kv=%d)", "H_kv must divide H (got H=%d, H_kv=%d)"]
    for m in re.finditer(r"fa2_set_error\(", src):
        pos, fmt = m.end(), ""
        while True:
            lit = re.compile(r'\s*"((?:[^"\\]|\\.)*)"').match(src, pos)
            if not lit:
                break
            fmt, pos = fmt + lit.group(1), lit.end()
        formats.append(fmt)
    return [(f, re.compile("^" + re.sub(r"%(?:lld|d|s)", ".*", re.escape(f).replace("%%", "%")) + "$")) for f in formats]


def unreached(result):
    """The sites no single's message matches."""
    seen = {result["messages"][r[1]] for v in result["singles"].values() for r in v}
    return [f for f, rx in error_sites() if not any(rx.match(m) for m in seen)]


def _library():
    """The library, only once the process is known to see no device."""
    import torch
    if torch.cuda.device_count() != 0:
        return None
    from flash_attention_dlrs_amd import _lib
    return _lib.lib()


def main(argv):
    if argv[1:] not in (["--record"], ["--replay"]):
        sys.exit(__doc__)
    lib = _library()
    if lib is None:
        print(json.dumps({"skipped": "a device is visible"}))
        return
    got = run(lib)
    if argv[1] == "--replay":
        with open(FIXTURE) as f:
            want = json.load(f)
        print(json.dumps({"mismatches": mismatches(want, got), "counts": counts(want)}))
        return
    with open(FIXTURE, "w") as f:
        json.dump(got, f, separators=(",", ":"))
        f.write("\n")
    c = counts(got)
    print(f"{FIXTURE}: {os.path.getsize(FIXTURE)} bytes; singles {sum(c['singles'].values())}, pairs {sum(c['pairs'].values())}, "
          f"valid {c['valid_stored']}, helper points {sum(c['helpers'].values())}")
    for f in unreached(got):
        print("no single reaches:", f)


if __name__ == "__main__":
    main(sys.argv)
