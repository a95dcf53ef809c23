#!/usr/bin/env python3
"""Packed (ragged) queries over the latent cache (fa2_fwd_kvcache_mla_varlen: d = 576, d_v = 512), bf16 Q, H_kv = 1, causal; JSON
lines appended to profiles/mla/bench_mla_varlen.jsonl.  --kv-dtype e4m3: the same shapes and sides over an fp8 latent cache with its
per-sequence descale.  The protocol is benchmarks/bench_mla_decode.py's: kernel times come from a `rocprofv3 --kernel-trace --stats`
child per shape (a fresh process, under its own `timeout -k 10`; the first non-zero status ends the run), every side rotates over
enough copies of the latent cache to exceed the 256 MiB last-level cache, each side is warmed (3 calls, not counted) and then run
back to back, and avg, min-max and stddev are reported per call.

Shapes (H in {16, 128}):
  verify2   draft verification: 64 sequences x 2 query tokens over 2048 keys;
  verify4   ... 16 sequences x 4 query tokens over 4096 keys;
  mixed     a mixed step: one 256-token prefill chunk over 4096 keys beside 63 one-token decodes over 2048;
  uniform1  the uniform one-token batch: 64 sequences x 1 token over 2048 keys;
  long4     one sequence x 4 query tokens over 8192 keys: the few-workgroup end of the split heuristic.

Sides of one child:
  auto       the packed call, AUTO variant, auto num_splits (fa2_kvcache_mla_varlen_num_splits);
  generic    the same launch with the VALU form forced, the same num_splits;
  padded     what a caller does without the packed call: the fixed call (fa2_fwd_kvcache_mla / _mla_fp8, AUTO, its own auto
             num_splits) on Q padded to N_q = max_seqlen_q for every sequence;
  per_count  ... or one fixed call per distinct query count, on views of the sequences that have it (a uniform batch: one call,
             the padded one).
The kernel trace is cut into the sides by dispatch order (split kernel plus combine per launch; one kernel for num_splits = 1).

Records:
  kind=kernels        one per shape: the sides' avg / min / max / stddev in microseconds, auto_over_generic, auto_over_padded,
                      auto_over_per_count and whether AUTO's and generic's min-max ranges overlap;
  kind=sweep_kernels  --sweep: AUTO's variant under num_splits in SWEEP_SPLITS, one traced child per shape."""
import argparse
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_mla_decode import D, D_V, emit, per_call, trace_rows  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "mla", "bench_mla_varlen.jsonl")
KV_DTYPES = ("bf16", "e4m3")
SWEEP_SPLITS = (1, 2, 4, 8, 16, 32, 64, 128)

# name -> [(sequences, n_q, N_k), ...]: the groups of one ragged batch, in batch order
BATCHES = {"verify2": [(64, 2, 2048)], "verify4": [(16, 4, 4096)], "mixed": [(1, 256, 4096), (63, 1, 2048)], "uniform1": [(64, 1, 2048)],
           "long4": [(1, 4, 8192)]}
CASES = {f"{name}_h{H}": (name, H) for name in BATCHES for H in (16, 128)}


class Case:
    def __init__(self, name, dev, kv_dtype="bf16"):
        import torch
        import flash_attention_dlrs_amd as fa
        from flash_attention_dlrs_amd import _lib
        from flash_attention_dlrs_amd.flash_attention_torch import convert_triton_dtype
        self.torch, self._lib, self.dev = torch, _lib, dev
        batch, H = CASES[name]
        self.groups = BATCHES[batch]
        n_q = [q for cnt, q, _ in self.groups for _ in range(cnt)]
        n_k = [k for cnt, _, k in self.groups for _ in range(cnt)]
        self.B, self.H, self.total_q, self.max_q, self.S = len(n_q), H, sum(n_q), max(n_q), max(n_k)
        self.shape = dict(B=self.B, H=H, total_q=self.total_q, max_seqlen_q=self.max_q, S_k=self.S, keys=sum(n_k),
                          score_rows_x_keys=H * sum(q * k for q, k in zip(n_q, n_k)))
        self.fmt = {"bf16": None, "e4m3": torch.float8_e4m3fn}[kv_dtype]
        self.kv_bytes = (1 if self.fmt else 2) * D * sum(n_k)  # the bytes of the visible keys, once
        self.copies = max(2, math.ceil(300e6 / ((1 if self.fmt else 2) * D * self.B * self.S)))
        self.scale = D ** -0.5
        self.enum = convert_triton_dtype(torch.bfloat16)
        mk = lambda *s: (torch.randn(*s, device=dev) * 0.8).to(torch.bfloat16)  # noqa: E731
        self.Q = mk(self.total_q, H, D)
        self.Qpad = mk(self.B, H, self.max_q, D)
        self.KV = [mk(self.B, 1, self.S, D) for _ in range(self.copies)]
        self.descale, self.kv_enum = None, self.enum
        if self.fmt:
            quant = [fa.quantize_kv_cache(t, self.fmt) for t in self.KV]
            self.KV, self.descale = [q[0] for q in quant], [q[1] for q in quant]
            self.kv_enum = convert_triton_dtype(self.fmt)
        self.cu = torch.tensor([0] + torch.tensor(n_q).cumsum(0).tolist(), dtype=torch.int32, device=dev)
        self.lens = torch.tensor(n_k, dtype=torch.int32, device=dev)
        self.O = torch.empty(self.total_q, H, D_V, dtype=torch.bfloat16, device=dev)
        self.L = torch.empty(H, self.total_q, dtype=torch.bfloat16, device=dev)
        self.i = 0

    def auto_splits(self):
        return self._lib.kvcache_mla_varlen_num_splits(self.B, self.H, 1, self.total_q, self.max_q, self.S, D, D_V, self.enum)

    def _next(self):
        self.i = (self.i + 1) % self.copies
        return self.KV[self.i], (self.descale[self.i] if self.fmt else None)

    def packed(self, variant, num_splits=0):
        """-> (run, [num_splits of each launch]): the library launch itself, outputs and workspace allocated once"""
        n = num_splits or self.auto_splits()
        ws = self.torch.empty(max(self._lib.kvcache_varlen_workspace_bytes(self.total_q, self.H, D_V, n) // 4, 1), dtype=self.torch.float32,
                              device=self.dev)

        def run():
            kv, ds = self._next()
            self._lib.fa2_fwd_kvcache_mla_varlen(self.Q, kv, self.O, self.L, self.cu, self.max_q, self.lens, self.enum, self.kv_enum, D_V,
                                                 kv_descale=ds, causal=True, scale=self.scale, num_splits=n, workspace=ws,
                                                 variant=self._lib.KVCACHE_MLA_VARIANTS[variant])
        return run, [n]

    def _fixed(self, first, count, n_q):
        """one fixed call on sequences [first, first + count) at N_q = n_q: views of the cache, Q and the lengths"""
        torch, lib = self.torch, self._lib
        n = lib.kvcache_mla_num_splits(count, self.H, 1, n_q, self.S, D, D_V, self.enum)
        ws = torch.empty(max(lib.kvcache_workspace_bytes(count, self.H, n_q, D_V, n) // 4, 1), dtype=torch.float32, device=self.dev)
        Q = self.Qpad[first:first + count, :, :n_q]
        O = torch.empty(count, self.H, n_q, D_V, dtype=torch.bfloat16, device=self.dev)
        L = torch.empty(count, self.H, n_q, dtype=torch.bfloat16, device=self.dev)
        lens = self.lens[first:first + count]

        def run(kv, ds):
            kv = kv[first:first + count]
            if self.fmt:
                ds = ds[first:first + count]
                lib.fa2_fwd_kvcache_mla_fp8(Q, kv, kv[..., :D_V], O, L, lens, self.enum, self.kv_enum, k_descale=ds, v_descale=ds,
                                            causal=True, scale=self.scale, num_splits=n, workspace=ws)
            else:
                lib.fa2_fwd_kvcache_mla(Q, kv, kv[..., :D_V], O, L, lens, self.enum, causal=True, scale=self.scale, num_splits=n, workspace=ws)
        return run, n

    def fixed(self, per_count):
        calls, first = [], 0
        if per_count:
            for cnt, q, _ in self.groups:
                calls.append(self._fixed(first, cnt, q))
                first += cnt
        else:
            calls.append(self._fixed(0, self.B, self.max_q))

        def run():
            kv, ds = self._next()
            for f, _ in calls:
                f(kv, ds)
        return run, [n for _, n in calls]


def kernels_of(splits):
    return sum(1 if n == 1 else 2 for n in splits)


def generic_iters(shape, iters):
    """the VALU form reads the keys once per query head: fewer calls where one takes tens of milliseconds"""
    return max(3, min(iters, int(2e8 / shape["score_rows_x_keys"])))


def run_pass(name, args):
    """The traced child: each side warmed, then run back to back; the kernel trace holds the times."""
    import torch
    c = Case(name, torch.device("cuda:0"), args.kv_dtype)
    sides = [("auto", c.packed("auto"), args.iters + 3), ("generic", c.packed("generic"), generic_iters(c.shape, args.iters) + 3),
             ("padded", c.fixed(False), args.iters + 3), ("per_count", c.fixed(True), args.iters + 3)]
    for _, (f, _), calls in sides:
        for _ in range(calls):
            f()
        torch.cuda.synchronize()
    print(json.dumps(dict(case=name, kv_dtype=args.kv_dtype, kv_bytes=c.kv_bytes, num_splits=c.auto_splits(),
                          sides=[(side, kernels_of(splits), calls, splits) for side, (_, splits), calls in sides], **c.shape)))


def run_sweep_pass(name, args):
    """The traced child of the split sweep: AUTO's variant alone, one split count after the other."""
    import torch
    c = Case(name, torch.device("cuda:0"), args.kv_dtype)
    for n in SWEEP_SPLITS:
        f, _ = c.packed("auto", n)
        for _ in range(args.iters + 3):
            f()
        torch.cuda.synchronize()
    print(json.dumps(dict(case=name, calls=args.iters + 3, kv_dtype=args.kv_dtype, auto_splits=c.auto_splits(), **c.shape)))


def child(out, extra, args):
    os.makedirs(out, exist_ok=True)
    cmd = ["timeout", "-k", "10", str(args.child_timeout), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out,
           "--", sys.executable, os.path.abspath(__file__), "--iters", str(args.iters), "--kv-dtype", args.kv_dtype] + extra
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode != 0:  # a failed child ends the run: nothing more is started on the GPU
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
        sys.exit(p.returncode)
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def run_rocprof(names, args, fh):
    suffix = "" if args.kv_dtype == "bf16" else "_" + args.kv_dtype
    for name in names:
        out = os.path.join(args.rocprof, "varlen_" + name + suffix)
        info = child(out, ["--pass-case", name], args)
        rows = [r for r in trace_rows(out) if "fa2_decode" in r["Kernel_Name"]]
        pos, sides = 0, {}
        for side, per, calls, splits in info.pop("sides"):
            sides[side] = dict(per_call(rows[pos:pos + per * calls], per, calls), launch_splits=splits)
            pos += per * calls
        assert pos == len(rows), (pos, len(rows))
        a, g = sides["auto"], sides["generic"]
        emit(fh, kind="kernels", **info, auto_over_generic=round(a["avg_us"] / g["avg_us"], 4), ranges_overlap=a["max_us"] >= g["min_us"],
             auto_over_padded=round(a["avg_us"] / sides["padded"]["avg_us"], 4),
             auto_over_per_count=round(a["avg_us"] / sides["per_count"]["avg_us"], 4), **sides)
        if args.sweep:
            out = os.path.join(args.rocprof, "varlen_" + name + "_sweep" + suffix)
            info = child(out, ["--sweep-case", name], args)
            rows = [r for r in trace_rows(out) if "fa2_decode" in r["Kernel_Name"]]
            pos, calls = 0, info["calls"]
            for n in SWEEP_SPLITS:
                per = 1 if n == 1 else 2
                emit(fh, kind="sweep_kernels", case=name, kv_dtype=args.kv_dtype, num_splits=n, auto_splits=info["auto_splits"],
                     **per_call(rows[pos:pos + per * calls], per, calls))
                pos += per * calls
            assert pos == len(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--sweep", action="store_true", help="also time AUTO's variant under num_splits in %s" % (SWEEP_SPLITS,))
    ap.add_argument("--rocprof", metavar="DIR", default=os.path.join(ROOT, "bench_out", "mla_traces"),
                    help="the traces of the rocprofv3 children go under DIR")
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--kv-dtype", choices=KV_DTYPES, default="bf16", help="the latent cache's storage: bf16, or fp8 with its descale")
    ap.add_argument("--pass-case", help=argparse.SUPPRESS)
    ap.add_argument("--sweep-case", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    if args.pass_case:
        return run_pass(args.pass_case, args)
    if args.sweep_case:
        return run_sweep_pass(args.sweep_case, args)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fh:
        run_rocprof(args.cases.split(","), args, fh)


if __name__ == "__main__":
    main()
