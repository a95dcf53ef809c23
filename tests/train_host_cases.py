"""The host path of training attention (csrc/fa2_api.hip, csrc/fa2_bwd_api.hip) as a deterministic list of calls through the raw
ctypes library with fake pointers: what tests/golden/train_host_calls.json records and tests/test_train_host_golden.py replays.  Not
collected by pytest.  Built like tests/decode_host_cases.py, whose helpers it imports.  Four kinds of case over the twenty launching
entry points (fa2_fwd / fa2_bwd, each plain, _window, _gqa, _varlen and _varlen_gqa, each with its _variant twin):

  singles  a valid base call with one argument (or one group of arguments) made wrong: the code and the whole message;
  pairs    every two singles of one entry point that change different arguments, in one call: which of the two results comes
           back (0 / 1), or the whole result where it is neither: this pins the order of the checks;
  valid    calls that pass every check and steer the dispatch, each with the table's choice and with a forced variant.  A process
           that sees no device gets FA2_ERR_LAUNCH from the first launch attempted, whose message names the kernel: the text is kept
           up to "launch failed" (the generated kernels fail earlier, at their code object: that text is kept whole).  The message
           does not tell a windowed or GQA form of a kernel from the plain one, so every base is also called with a variant its
           tail does not take (mfma16h forward, mfma32 backward): the refusal names the tail that was reached;
  helpers  fa2_query_tile_scaled over a grid of (B, H, N, d, dtype, causal, scale) -- both sides of every threshold of pick_variant,
           at the 256 CUs the library assumes without a device -- and fa2_query_tile / fa2_query_tile_ex at a few points: all four
           integers of every point, stored as an index into the list of distinct results.

    python tests/train_host_cases.py --record     writes the fixture from the library in the tree (and prints the fa2_set_error
                                                  sites of the two files that no single reached)
    python tests/train_host_cases.py --replay     prints one JSON line: {"skipped": ...} or {"mismatches": [...], "counts": ...}

Both refuse to make a library call while a device is visible (start them with HIP_VISIBLE_DEVICES=-1): a call that passes the
checks would otherwise launch on a fake pointer.

Every fa2_set_error site of the two files is reached by a single, "out4 is null" of fa2_query_tile_scaled by a helper case.  The
two `!fits32` returns of pick_variant: the query reaches MFMA16_W8 at N = 2^23, d = 128; MFMA16 needs fewer than 512 256-row tiles
with a row stride of 2 GiB / N, which a contiguous problem cannot have, so a valid call with a K row stride of 2^22 records it."""
import ctypes
import hashlib
import itertools
import json
import os
import re
import sys

from decode_host_cases import BF16, F16, F32, F64, F8E4, F8E5, NAN, ROOT, P, _array, _library, contiguous, join

FIXTURE = os.path.join(ROOT, "tests", "golden", "train_host_calls.json")
SOURCES = [os.path.join(ROOT, "flash_attention_dlrs_amd", "csrc", f) for f in ("fa2_api.hip", "fa2_bwd_api.hip", "fa2_host.h")]

# FA2_VARIANT_* of include/fa2_fwd.h (the forward's product kernels) and FA2_BWD_VARIANT_*
FWD_IDS = dict(GENERIC=1, MFMA16=2, MFMA16_W8=3, MFMA32=4, MFMA16D=8, MFMA16D_W4=9, MFMA16H=14, MFMA16H_W4=15, MFMA8X=16, MFMA8X_W4=17,
               MFMA16K=19, MFMA16K_R2K2=20, MFMA16K_R2K4=23, A64=24, A16=25, A8=26, A64D=27)
BWD_IDS = dict(GENERIC=1, MFMA16=2, MFMA32=3)
# what the query grid must return at least once: every `return` of pick_variant
PICKED = ("GENERIC MFMA16 MFMA16_W8 MFMA32 A64D A64 A16 A8 MFMA16K MFMA16K_R2K2 MFMA16K_R2K4 MFMA16D_W4 MFMA16H MFMA8X "
          "MFMA8X_W4").split()

_FWD_T, _BWD_T = "Q K V O L", "Q K V O dO L dQ dK dV D"
_FWD_S = "q_strides k_strides v_strides o_strides"
_BWD_S = _FWD_S + " do_strides dq_strides dk_strides dv_strides"
_WIN = "window_left window_right"


def _orders(prefix, tensors, strides):
    """The parameters of the ten entry points of one direction, in the header's order."""
    dense = lambda sizes, win: f"{tensors} {strides} l_strides {sizes} dtype_enum causal scale {win} hip_stream"
    packed = lambda heads: (f"{tensors} {strides} l_head_stride cu_seqlens_q cu_seqlens_k B {heads} d max_seqlen_q max_seqlen_k total_q "
                            f"total_k dtype_enum causal scale {_WIN} hip_stream")
    forms = {"": dense("B H N d", ""), "_window": dense("B H N d", _WIN), "_gqa": dense("B H H_kv N d", _WIN),
             "_varlen": packed("H"), "_varlen_gqa": packed("H H_kv")}
    out = {}
    for form, order in forms.items():
        out[prefix + form] = order.split()
        out[prefix + form + "_variant"] = order.split() + ["variant"]
    return out


ORDER = join(_orders("fa2_fwd", _FWD_T, _FWD_S), _orders("fa2_bwd", _BWD_T, _BWD_S))
ENTRY_POINTS = tuple(ORDER)
_Q_LIKE, _K_LIKE = ("q_strides", "o_strides", "do_strides", "dq_strides"), ("k_strides", "v_strides", "dk_strides", "dv_strides")


def _shape(B=2, H=8, N=512, d=64, H_kv=None):
    """A dense call at another shape, contiguous (H_kv: of the GQA entry points)."""
    q, k = contiguous(B, H, N, d), contiguous(B, H_kv or H, N, d)
    out = join({s: q for s in _Q_LIKE}, {s: k for s in _K_LIKE}, B=B, H=H, N=N, d=d, l_strides=(H * N, N))
    return join(out, H_kv=H_kv) if H_kv else out


def _packed_shape(H=8, d=64, H_kv=None, total=700):
    q, k = contiguous(total, H, d), contiguous(total, H_kv or H, d)
    out = join({s: q for s in _Q_LIKE}, {s: k for s in _K_LIKE}, H=H, d=d, total_q=total, total_k=total, l_head_stride=total)
    return join(out, H_kv=H_kv) if H_kv else out


# A base call per entry point that passes every check: B 2, H 8 (H_kv 2), N 512, d 64, bf16; packed: 3 sequences of at most 300 rows
# in 700.  A case is a dict of replacements; the names an entry point does not have are left out of its call.
_COMMON = join({t: P for t in _BWD_T.split()}, dtype_enum=BF16, causal=0, scale=1.0, window_left=-1, window_right=-1, hip_stream=None,
               variant=0)
BASE = {}
for _name in ENTRY_POINTS:
    _kv = 2 if "_gqa" in _name else None
    BASE[_name] = join(_COMMON, _packed_shape(H_kv=_kv), B=3, cu_seqlens_q=0x5000, cu_seqlens_k=0x5100, max_seqlen_q=300,
                       max_seqlen_k=300) if "_varlen" in _name else join(_COMMON, _shape(H_kv=_kv))

BAND = dict(window_left=64, window_right=0)  # a window that does not reduce to plain or causal attention
ODD_K = dict(k_strides=(2 * 512 * 64 + 64, 512 * 64, 64, 1))  # a dense GQA layout the host cannot merge (base shape, H_kv 2)
WIDE_K = 1 << 22  # a K row stride that fails the 32-bit offset rule of the LDS-DMA kernels at any N


def _has(name, arg):
    return arg in ORDER[name]


def _forced(name):
    """A variant id that exists but that no windowed, varlen or GQA tail takes."""
    return BWD_IDS["MFMA32"] if name.startswith("fa2_bwd") else FWD_IDS["MFMA16H"]


def singles(name):
    o, bwd, packed = ORDER[name], name.startswith("fa2_bwd"), "_varlen" in name
    tensors, strides = [a for a in o if a in _BWD_T.split()], [a for a in o if a.endswith("_strides")]
    s = [{a: None} for a in tensors + strides]
    s += [dict(B=0), dict(B=-1), dict(H=0), dict(d=0), dict(dtype_enum=99), dict(scale=NAN)]
    s += [dict(d=48), dict(d=8), dict(d=1024), dict(dtype_enum=F8E4), dict(dtype_enum=F8E5)] if bwd else [dict(d=513)]
    neg = (64, -64, 1) if packed else (-1, 64, 64, 1)
    s += [{a: neg} for a in strides if a != "l_strides"]
    for a in ("dq_strides", "dk_strides", "dv_strides") if bwd else ("o_strides",):
        s += [{a: (512, 64, 0) if packed else (512 * 512, 512 * 64, 64, 0)}, {a: (0, 64, 1) if packed else (512 * 512, 512 * 64, 0, 1)}]
    if packed:
        s += [dict(cu_seqlens_q=None), dict(cu_seqlens_k=None), dict(B=65536), dict(H=65536), dict(max_seqlen_q=-1),
              dict(max_seqlen_k=(1 << 28) + 1), dict(total_q=-1), dict(total_k=-2), dict(l_head_stride=-1)]
        if not bwd:
            s += [dict(dtype_enum=F8E4), dict(dtype_enum=F8E5)]
    else:
        s += [dict(N=0), dict(N=-5)]
    if _has(name, "window_left"):
        s += [dict(window_left=-2), dict(window_right=-5)]
    if _has(name, "H_kv"):
        s += [dict(H_kv=0), dict(H_kv=-1), dict(H_kv=3)]
    if _has(name, "variant"):
        s += [dict(variant=99), dict(variant=-1), dict(variant=5)]
        # a variant the tail does not take (the plain calls take every id of their table)
        if packed:
            s += [dict(variant=_forced(name))]
        elif _has(name, "H_kv"):
            s += [dict(ODD_K, variant=_forced(name)), dict(BAND, variant=_forced(name))]
        elif _has(name, "window_left"):
            s += [dict(BAND, variant=_forced(name))]
    for c in s:
        assert set(c) <= set(o), (name, c)
    return s


def pairs(name):
    """(i, j, the two singles in one call) for every two singles of `name` that change different arguments."""
    s = singles(name)
    return [(i, j, dict(s[i], **s[j])) for i, j in itertools.combinations(range(len(s)), 2) if not set(s[i]) & set(s[j])]


def _steer(name):
    """The replacements that steer entry point `name` (either twin) past its checks into different launches."""
    bwd = name.startswith("fa2_bwd")
    if "_varlen" in name:
        kv = 2 if "_gqa" in name else None
        wide = join({a: (WIDE_K, 64, 1) for a in _K_LIKE})
        out = [{}, dict(causal=1), dict(BAND), dict(window_left=-1, window_right=5), dict(max_seqlen_q=0), dict(max_seqlen_k=0),
               dict(max_seqlen_q=0, max_seqlen_k=0), dict(total_q=0, total_k=0), dict(dtype_enum=F16), dict(dtype_enum=F32), dict(dtype_enum=F64),
               _packed_shape(d=128, H_kv=kv), dict(Q=0x1004), dict(scale=0.0), wide, dict(wide, max_seqlen_q=0), dict(max_seqlen_q=1 << 28)]
        if not bwd:
            out += [_packed_shape(d=40, H_kv=kv), _packed_shape(d=3, H_kv=kv)]
        if kv:
            out += [_packed_shape(H_kv=8), _packed_shape(H_kv=1), dict(_packed_shape(H_kv=1), max_seqlen_q=0)]
        return out
    kv = 2 if "_gqa" in name else None
    wide = {a: (0, 0, WIDE_K, 1) for a in _K_LIKE}
    shapes = [{}, dict(dtype_enum=F16), dict(dtype_enum=F32), dict(dtype_enum=F64), _shape(d=128, H_kv=kv), _shape(B=16, H_kv=kv),
              _shape(B=64, N=4096, d=128, H_kv=kv), _shape(B=8, H=16, N=4096, H_kv=kv), dict(_shape(d=128, H_kv=kv), dtype_enum=F32),
              dict(Q=0x1004), dict(K=0x1008), dict(scale=0.0), dict(scale=0.5, dtype_enum=F16), wide, dict(_shape(d=128, H_kv=kv), **wide),
              _shape(N=1, H_kv=kv), dict(q_strides=(8 * 512 * 128, 512 * 128, 128, 2))]
    if not bwd:
        shapes += [_shape(d=40, H_kv=kv), _shape(d=3, H_kv=kv), dict(_shape(B=64, N=2048, d=128, H_kv=kv), dtype_enum=F8E4),
                   dict(_shape(d=128, H_kv=kv), dtype_enum=F8E5)]
    if not _has(name, "window_left"):
        return shapes + [dict(c, causal=1) for c in shapes[:8]]
    # windows: that reduce to plain (unbounded, N - 1 or more), to causal, and true bands
    windows = [dict(window_left=-1, window_right=-1), dict(window_left=511, window_right=511), dict(window_left=600, window_right=-1),
               dict(window_left=511, window_right=0), dict(window_left=-1, window_right=0), dict(window_left=-1, window_right=7, causal=1),
               dict(window_left=510, window_right=511), BAND, dict(window_left=64, window_right=64), dict(window_left=0, window_right=0),
               dict(window_left=-1, window_right=64), dict(window_left=64, window_right=-1, causal=1)]
    out = [dict(c, **w) for c in shapes[:6] + shapes[9:10] + shapes[13:16] for w in windows]
    out += [dict(c, **w) for c in shapes[6:9] + shapes[10:13] + shapes[16:] for w in (windows[0], windows[4], BAND)]
    if kv:
        layouts = [dict(_shape(B=1, H_kv=2), q_strides=(8, 512 * 64, 64, 1), k_strides=(16, 512 * 64, 64, 1)),            # B == 1: merges
                   dict(_shape(H_kv=1), k_strides=(512 * 64, 8, 64, 1), v_strides=(512 * 64, 24, 64, 1)),                 # free head stride
                   ODD_K, dict(q_strides=(8 * 512 * 64 + 64, 512 * 64, 64, 1)), dict(l_strides=(8 * 512 + 8, 512)),     # do not merge
                   dict(_shape(H_kv=1), v_strides=(512 * 64 + 64, 8, 64, 1)), _shape(H_kv=8), _shape(H_kv=4, N=1),
                   # B * H_kv > 65535: stays unmerged where the table picks the generic kernel, whose grid could not hold it
                   dict(_shape(B=40000, H=4, N=16, d=32, H_kv=2), dtype_enum=F64), dict(_shape(B=40000, H=4, N=16, d=32, H_kv=2), dtype_enum=F32),
                   _shape(B=40000, H=4, N=16, H_kv=2), dict(_shape(B=32768, H=4, N=16, d=32, H_kv=2), dtype_enum=F64),
                   dict(_shape(B=21845, H=6, N=16, d=32, H_kv=3), dtype_enum=F64),
                   _shape(B=40000, H=4, N=16, d=32, H_kv=2), dict(_shape(B=1 << 30, H=8, N=16, d=32, H_kv=4), dtype_enum=F32)]
        out += [dict(c, **w) for c in layouts for w in (windows[0], windows[4], BAND, dict(window_left=3, window_right=3))]
        out += [dict(c, dtype_enum=F32, **w) for c in layouts[:6] for w in (windows[0], BAND)]
    return out


def valid():
    """(entry point, replacements): calls that pass every check, chosen to steer the dispatch."""
    out = []
    for name in ENTRY_POINTS:
        if name.endswith("_variant"):
            continue
        ids = BWD_IDS if name.startswith("fa2_bwd") else FWD_IDS
        for c in _steer(name):
            c = {k: v for k, v in c.items() if k in ORDER[name]}
            out += [(name, c), (name + "_variant", c), (name + "_variant", dict(c, variant=_forced(name)))]
        # every id on a problem it could run: the launcher each row of the tables names
        big = {k: v for k, v in _shape(B=64, N=4096, d=128, H_kv=2 if "_gqa" in name else None).items() if k in ORDER[name]}
        for c in ([big, dict(big, **BAND), dict(big, **ODD_K)] if "_varlen" not in name else [{}]):
            c = {k: v for k, v in c.items() if k in ORDER[name]}
            out += [(name + "_variant", dict(c, variant=v)) for v in ids.values()]
    return out


def tile_grid():
    """(B, H, N, d, dtype, causal, scale) of the fa2_query_tile_scaled grid."""
    marks = (64, 96, 128, 160, 192, 224, 256, 320, 384, 448, 512)  # the T(n) of pick_variant's rules, in 256- or 128-row tiles
    jobs = (153, 154, 384, 426, 427, 512, 640)                     # its `even` rule: 0.6, 1.5, 1.67, 2 and 2.5 jobs per CU
    kinds = [(BF16, 64, 1.0), (BF16, 128, 1.0), (F16, 64, 1.0), (F16, 128, 1.0), (F16, 64, 0.5), (F16, 128, 0.5), (F8E4, 128, 1.0)]
    # ... and the kinds whose only rule is T(160) or T(512)
    rest = [(F16, 128, 0.75), (F8E5, 128, 1.0), (F32, 128, 1.0), (F32, 64, 1.0), (BF16, 40, 1.0), (BF16, 96, 1.0)]
    pts = []
    for N in (128, 200, 256, 300, 512, 1024, 2048, 4096, 8192):
        t256, t128 = (N + 255) // 256, (N + 127) // 128
        for causal in (0, 1):
            per = {t256, t128, (t256 + 1) // 2 if causal else t256, t128 // 2 if causal and t128 > 1 else t128}
            bh = {max(1, -(-m // t) + e) for m in marks + jobs for t in per for e in (-1, 0, 1)}
            pts += [(b, 1, N, d, dt, causal, sc) for dt, d, sc in kinds for b in sorted(bh)]
            pts += [(max(1, -(-m // t256) + e), 1, N, d, dt, causal, sc) for dt, d, sc in rest for m in (160, 512) for e in (-1, 0, 1)]
    # B and H apart, sizes off the table, the 32-bit rule (N x row stride >= 2 GiB), and what the query refuses
    pts += [(4, 16, 4096, 128, BF16, 1, 1.0), (64, 8, 4096, 128, BF16, 0, 1.0), (1, 1, 1 << 23, 128, BF16, 0, 1.0), (1, 1, 1 << 23, 128, F16, 1, 1.0),
            (1, 1, (1 << 23) - 1024, 128, BF16, 0, 1.0), (1, 1, 1 << 24, 64, BF16, 0, 1.0), (1, 1, (1 << 24) + 1, 64, BF16, 0, 1.0),
            (1, 1, 1 << 24, 128, F8E4, 0, 1.0), (2, 8, 512, 3, F32, 0, 1.0), (2, 8, 512, 4, F32, 0, 1.0), (2, 8, 512, 8, BF16, 0, 1.0),
            (2, 8, 512, 256, BF16, 0, 1.0), (2, 8, 512, 512, F64, 0, 1.0), (2, 8, 512, 64, F64, 1, 1.0), (2, 8, 512, 64, F8E4, 0, 1.0),
            (2, 8, 1, 64, BF16, 0, 1.0), (2, 8, 512, 64, BF16, 0, 0.0), (2, 8, 512, 64, BF16, 0, -1.0), (2, 8, 512, 64, BF16, 0, float("inf")),
            (2, 8, 512, 64, BF16, 0, NAN), (0, 8, 512, 64, BF16, 0, 1.0), (2, 0, 512, 64, BF16, 0, 1.0), (2, 8, 0, 64, BF16, 0, 1.0),
            (2, 8, 512, 0, BF16, 0, 1.0), (2, 8, 512, 513, BF16, 0, 1.0), (2, 8, 512, 64, 99, 0, 1.0)]
    return pts


def helpers():
    """(function, argument tuples without the output array)."""
    few = [(N, d, dt, causal) for N in (128, 512, 4096, 16384) for d, dt in ((64, BF16), (128, F16), (128, F8E4), (128, F32), (48, F64))
           for causal in (0, 1)] + [(0, 64, BF16, 0), (512, 64, 99, 0)]
    return [("fa2_query_tile_scaled", tile_grid()), ("fa2_query_tile", few),
            ("fa2_query_tile_ex", [(B, H) + p for B, H in ((64, 8), (1, 1), (2, 16)) for p in few])]


def call(lib, name, case):
    """(code, message) of entry point `name` at its base call with `case`'s replacements.  The message of a launch failure ends at
    "launch failed": what follows is the runtime's wording."""
    a = dict(BASE[name], **case)
    rc = getattr(lib, name)(*[_array(a[p]) if p.endswith("_strides") else a[p] for p in ORDER[name]])
    msg = lib.fa2_last_error().decode()
    cut = msg.find("launch failed")
    return [rc, msg if cut < 0 else msg[:cut + len("launch failed")]]


def query(lib, name, args, null=False):
    """[variant, B_r, B_c, waves] of a tile query, or [code, message] where it refuses."""
    out4 = (ctypes.c_int32 * 4)()
    rc = getattr(lib, name)(*args, None if null else out4)
    return list(out4) if rc == 0 else [rc, lib.fa2_last_error().decode()]


def digest():
    """Of the case lists: a fixture recorded from another generator is refused instead of compared case by case."""
    text = repr([(n, singles(n)) for n in ENTRY_POINTS]) + repr(valid()) + repr(helpers())
    return hashlib.sha256(text.encode()).hexdigest()[:16]


def run(lib):
    """Every case against `lib`, in the fixture's form.  Messages are stored once, in "messages"; a result is [code, index].  The
    helpers' results are stored once in "tiles"; a grid is a list of indices into it."""
    messages, tiles = {}, {}
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
        out["helpers"][name] = [tiles.setdefault(json.dumps(query(lib, name, args)), len(tiles)) for args in grid]
    out["null_out4"] = ref(query(lib, "fa2_query_tile_scaled", (2, 8, 512, 64, BF16, 0, 1.0), null=True))
    out["messages"], out["tiles"] = list(messages), [json.loads(t) for t in tiles]
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
            if want["tiles"][w] != got["tiles"][g]:
                bad.append(f"helper {name}{args}: want {want['tiles'][w]}, got {got['tiles'][g]}")
    if text(want, want["null_out4"]) != text(got, got["null_out4"]):
        bad.append(f"helper fa2_query_tile_scaled(out4 = null): want {text(want, want['null_out4'])}, got {text(got, got['null_out4'])}")
    return bad


def counts(fixture):
    return {"singles": {n: len(v) for n, v in fixture["singles"].items()}, "pairs": {n: len(v["which"]) for n, v in fixture["pairs"].items()},
            "valid": {n: sum(1 for m, _ in valid() if m == n) for n in ENTRY_POINTS}, "valid_stored": len(fixture["valid"]),
            "helpers": {n: len(v) for n, v in fixture["helpers"].items()}}


def picked(fixture):
    """The names of the variant ids the fa2_query_tile_scaled grid returned."""
    ids = {fixture["tiles"][k][0] for k in fixture["helpers"]["fa2_query_tile_scaled"] if len(fixture["tiles"][k]) == 4}
    return {n for n, v in FWD_IDS.items() if v in ids}


def error_sites():
    """The format strings of every fa2_set_error call of the two api files (and the header they share), as regular expressions."""
    formats = []
    for path in SOURCES:
        src = open(path).read()
        for m in re.finditer(r"fa2_set_error\(", src):
            pos, fmt = m.end(), ""
            while True:
                lit = re.compile(r'\s*"((?:[^"\\]|\\.)*)"').match(src, pos)
                if not lit:
                    break
                fmt, pos = fmt + lit.group(1), lit.end()
            if fmt:  # (not the definition of fa2_set_error itself, nor a call that passes a format on)
                formats.append(fmt)
    return [(f, re.compile("^" + re.sub(r"%(?:lld|d|s)", ".*", re.escape(f).replace("%%", "%")) + "$")) for f in dict.fromkeys(formats)]


def unreached(result):
    """The sites no single's message (nor the null-out4 query's) matches."""
    seen = {result["messages"][r[1]] for v in result["singles"].values() for r in v} | {result["messages"][result["null_out4"][1]]}
    return [f for f, rx in error_sites() if not any(rx.match(m) for m in seen)]


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
    for name in ENTRY_POINTS:  # a single fails a check: it neither passes nor reaches a launch
        for c, r in zip(singles(name), got["singles"][name]):
            assert r[0] in (-1, -2, -3), (name, c, r, got["messages"][r[1]])
    assert picked(got) >= set(PICKED), sorted(set(PICKED) - picked(got))
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
