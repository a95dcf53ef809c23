#!/usr/bin/env python3
"""MLA indexer timing (fa2_mla_indexer_topk: H_I = 64, d_I = 128, topk = 2048), bf16 q_idx over bf16 or e4m3 index keys; JSON lines
appended to profiles/mla/bench_mla_indexer.jsonl.  The protocol is benchmarks/bench_mla_sparse.py's: kernel times come from a
`rocprofv3 --kernel-trace --stats` child per shape (a fresh process, under its own `timeout -k 10`; the first non-zero status ends the
run), every side rotates over enough copies of the index-key cache to exceed the 256 MiB last-level cache, each side is warmed (3 calls,
not counted) and then run back to back, and avg, min-max and stddev are reported per call.  A one-element fill launched after every
call marks the call boundaries in the trace; it is not counted.

Sides of one child (causal, every sequence full):
  auto     fa2_mla_indexer_topk, AUTO variant (the matrix form on these shapes), scores and selection on one stream;
  generic  the same call, the VALU score kernel forced;
  torch    the only earlier route: einsum in q_idx's dtype over all keys (an e4m3 cache dequantised first), relu, the weighted sum over
           the heads, the scale, masked_fill, torch.topk -- all its kernels counted; it leaves int64 lists in no stated order.

Records (kind=kernels): per shape and key dtype the sides' avg / min / max / stddev in microseconds, for `auto` and `generic` the score
and the selection kernel apart (score_*, select_*), the ratios of AUTO to the other sides and whether the min-max ranges overlap; for a
prefill chunk the score kernel's TFLOP/s (2 H_I d_I per causal query-key pair)."""
import argparse
import csv
import glob
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "mla", "bench_mla_indexer.jsonl")
H_I, D_I, TOPK = 64, 128, 2048
K_DTYPES = ("bf16", "e4m3")
SHAPES = ((1, 65536), (16, 16384), (128, 8192))  # (B, N_k): the sparse table's
CASES = {f"q{N_q}_b{B}_n{S}": (B, N_q, S) for N_q in (1, 2) for B, S in SHAPES}
CASES["prefill_q1024_b1_n16384"] = (1, 1024, 16384)
MARK = "FillFunctor"
SELECT = "fa2_topk_indices_kernel"


def emit(fh, **kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if fh is not None:
        fh.write(line + "\n")
        fh.flush()


class Case:
    def __init__(self, name, dev, k_dtype="bf16"):
        import torch
        import flash_attention_dlrs_amd as fa
        from flash_attention_dlrs_amd import _lib
        from flash_attention_dlrs_amd.flash_attention_torch import convert_triton_dtype
        self.torch, self._lib, self.dev = torch, _lib, dev
        B, N_q, S = CASES[name]
        self.shape = dict(B=B, N_q=N_q, N_k=S, H_I=H_I, d_I=D_I, topk=TOPK)
        self.fmt = {"bf16": None, "e4m3": torch.float8_e4m3fn}[k_dtype]
        self.copies = max(2, math.ceil(300e6 / ((1 if self.fmt else 2) * D_I * B * S)))
        self.enum = convert_triton_dtype(torch.bfloat16)
        mk = lambda *s: torch.randn(*s, device=dev).to(torch.bfloat16)  # noqa: E731
        self.q = mk(B, H_I, N_q, D_I)
        self.w = torch.randn(B, H_I, N_q, device=dev) * H_I ** -0.5
        self.K = [mk(B, S, D_I) for _ in range(self.copies)]
        self.scale, self.k_enum = [None] * self.copies, self.enum
        if self.fmt:
            quant = [fa.quantize_index_keys(t, self.fmt) for t in self.K]
            self.K, self.scale = [x[0] for x in quant], [x[1] for x in quant]
            self.k_enum = convert_triton_dtype(self.fmt)
        self.lens = torch.full((B,), S, dtype=torch.int32, device=dev)
        self.logits = torch.empty(B, N_q, S, dtype=torch.float32, device=dev)
        self.indices = torch.empty(B, N_q, TOPK, dtype=torch.int32, device=dev)
        # the torch route's mask: key j is no candidate of query qi (causal, bottom-right)
        self.hidden = torch.arange(S, device=dev)[None, :] > (S - N_q + torch.arange(N_q, device=dev))[:, None]
        self.mark = torch.zeros(1, device=dev)
        self.i = 0

    def _next(self):
        self.i = (self.i + 1) % self.copies
        return self.K[self.i], self.scale[self.i]

    def indexer(self, variant):
        def run():
            k, ks = self._next()
            self._lib.fa2_mla_indexer_topk(self.q, self.w, k, ks, self.logits, self.indices, self.lens, self.enum, self.k_enum,
                                           causal=True, variant=self._lib.INDEXER_VARIANTS[variant])
        return run

    def torch_route(self):
        torch = self.torch
        wq = self.w.to(torch.bfloat16)[..., None]

        def run():
            k, ks = self._next()
            if self.fmt:
                k = k.to(torch.bfloat16)
            s = torch.einsum("bhqd,bkd->bhqk", self.q, k).relu_()
            lg = (s * wq).sum(1, dtype=torch.float32)
            if ks is not None:
                lg = lg * ks[:, None, :]
            self.out = torch.topk(lg.masked_fill_(self.hidden, float("-inf")), TOPK, dim=-1).indices
        return run


def side_iters(side, shape, iters):
    """the VALU form and the torch route take tens of milliseconds on the large shapes: fewer calls there"""
    work = shape["B"] * shape["N_q"] * shape["N_k"] * H_I * D_I
    return max(3, min(iters, int({"auto": 2e13, "torch": 4e12, "generic": 4e11}[side] / work)))


def timed(c, f, calls):
    for _ in range(calls):
        f()
        c.mark.fill_(1.0)
    c.torch.cuda.synchronize()


def run_pass(name, args):
    """The traced child: each side warmed, then run back to back; the kernel trace holds the times."""
    import torch
    c = Case(name, torch.device("cuda:0"), args.k_dtype)
    torch.cuda.synchronize()
    c.mark.fill_(0.0)  # the first marker: what lies before it is set-up
    sides = [("auto", c.indexer("auto")), ("generic", c.indexer("generic")), ("torch", c.torch_route())]
    calls = {}
    for side, f in sides:
        calls[side] = side_iters(side, c.shape, args.iters) + 3
        timed(c, f, calls[side])
    print(json.dumps(dict(case=name, calls=calls, order=[s for s, _ in sides], k_dtype=args.k_dtype, **c.shape)))


def traced_child(out, extra, args):
    os.makedirs(out, exist_ok=True)
    cmd = ["timeout", "-k", "10", str(args.child_timeout), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out,
           "--", sys.executable, os.path.abspath(__file__), "--iters", str(args.iters), "--k-dtype", args.k_dtype] + extra
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode != 0:  # a failed child ends the run: nothing more is started on the GPU
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
        sys.exit(p.returncode)
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def call_times(out, total):
    """per call of the last `total`: (kernel time, the selection kernel's share, kernel names), microseconds; the trace cut at the marks"""
    trace = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
    rows = sorted(csv.DictReader(open(trace[0])), key=lambda r: int(r["Start_Timestamp"]))
    marks = [k for k, r in enumerate(rows) if MARK in r["Kernel_Name"]][-(total + 1):]
    assert len(marks) == total + 1 and marks[-1] == len(rows) - 1, (len(marks), total, marks[-1], len(rows))
    calls = []
    for lo, hi in zip(marks, marks[1:]):
        seg = rows[lo + 1:hi]
        assert seg, "two marks with no kernel between them"
        us = lambda xs: sum(int(x["End_Timestamp"]) - int(x["Start_Timestamp"]) for x in xs) / 1e3  # noqa: E731
        calls.append((us(seg), us([x for x in seg if SELECT in x["Kernel_Name"]]), sorted({x["Kernel_Name"][:60] for x in seg})))
    return calls


def spread(us, prefix=""):
    avg = sum(us) / len(us)
    return {prefix + "avg_us": round(avg, 2), prefix + "min_us": round(min(us), 2), prefix + "max_us": round(max(us), 2),
            prefix + "stddev_us": round((sum((u - avg) ** 2 for u in us) / len(us)) ** 0.5, 2)}


def stats(calls, split, warm=3):
    rec = dict(spread([t for t, _, _ in calls[warm:]]), calls=len(calls) - warm, kernels=sorted({k for _, _, ks in calls for k in ks}))
    if split:
        rec.update(spread([t - s for t, s, _ in calls[warm:]], "score_"))
        rec.update(spread([s for _, s, _ in calls[warm:]], "select_"))
    return rec


def run_rocprof(names, args, fh):
    for name in names:
        out = os.path.join(args.rocprof, name + "_" + args.k_dtype)
        info = traced_child(out, ["--pass-case", name], args)
        calls = call_times(out, sum(info["calls"].values()))
        sides, pos = {}, 0
        for side in info["order"]:
            sides[side] = stats(calls[pos:pos + info["calls"][side]], side != "torch")
            pos += info["calls"][side]
        a = sides["auto"]
        extra = {}
        if info["N_q"] > 8:  # a prefill chunk: causal pairs only
            pairs = info["B"] * sum(info["N_k"] - info["N_q"] + qi + 1 for qi in range(info["N_q"]))
            extra["score_tflops"] = round(2 * H_I * D_I * pairs / (a["score_avg_us"] * 1e-6) / 1e12, 1)
        emit(fh, kind="kernels", **{k: v for k, v in info.items() if k not in ("calls", "order")},
             auto_over_torch=round(a["avg_us"] / sides["torch"]["avg_us"], 4), torch_ranges_overlap=a["max_us"] >= sides["torch"]["min_us"],
             auto_over_generic=round(a["avg_us"] / sides["generic"]["avg_us"], 4),
             generic_ranges_overlap=a["max_us"] >= sides["generic"]["min_us"], **extra, **sides)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rocprof", metavar="DIR", default=os.path.join(ROOT, "bench_out", "mla_indexer_traces"),
                    help="the traces of the rocprofv3 children go under DIR")
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--k-dtype", choices=K_DTYPES, default="bf16", help="the index keys' storage: bf16, or e4m3 with its per-row scale")
    ap.add_argument("--pass-case", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    if args.pass_case:
        return run_pass(args.pass_case, args)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fh:
        run_rocprof(args.cases.split(","), args, fh)


if __name__ == "__main__":
    main()
