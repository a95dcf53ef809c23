#!/usr/bin/env python3
"""Selection timing of the MLA indexer (fa2_topk_indices against fa2_topk_indices_split, topk = 2048): one workgroup a row against a
row split over 2 - 64 workgroups, the library's own choice and torch.topk; JSON lines appended to
profiles/mla/bench_topk_select.jsonl.  The protocol is benchmarks/bench_mla_indexer.py's (its trace reader is imported): kernel times
from a `rocprofv3 --kernel-trace --stats` child per shape (a fresh process under its own `timeout -k 10`; the first non-zero status
ends the run), no counters, 3 warm-up and 20 timed calls a side back to back, a one-element fill after every call as the boundary in
the trace, the logits buffers rotating over more than 256 MiB.  A call's time is the sum of its kernels (the split form: one clear,
four passes, one emit), not the gaps between them.

Cases.
  sel_r{rows}_n{N_k}            the selection alone: `rows` rows of N_k candidates each, the logits from the real score kernel
                                (mla_indexer_logits, H_I 64, d_I 128, bf16, non-causal) on N(0, 1) operands.
  sel_r1_n65536_equal, _ints7   data sensitivity: all values equal; seven integer values.
  whole_{bf16,e4m3}_q{1,2}      the whole indexer call on the four one-sequence rows of DESIGN.md "MLA indexer" (B 1, N_k 65,536,
                                causal): the fused call (one workgroup a row), the score call followed by the split selection at
                                the library's count, and bench_mla_indexer.py's torch route.

Sides of a selection case: s1 (fa2_topk_indices, the one-workgroup kernel), s2 .. s64 (the count forced), auto (num_splits = 0) and
torch (torch.topk, values and int64 lists in value order, all its kernels counted).  Records (kind=select / whole): per side avg / min
/ max / stddev in microseconds, every side's ratio to s1 and whether the min-max ranges overlap, and the count auto resolved to."""
import argparse
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "benchmarks"))
from bench_mla_indexer import Case as IndexerCase, call_times, emit, spread, timed  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "mla", "bench_topk_select.jsonl")
H_I, D_I, TOPK = 64, 128, 2048
COUNTS = (1, 2, 4, 8, 16, 32, 64)
CASES = {f"sel_r{r}_n{n}": (r, n, "score") for n in (8192, 16384, 65536, 163840) for r in (1, 2, 16, 32, 128, 1024) if n < 163840 or r <= 128}
CASES.update({f"sel_r1_n65536_{kind}": (1, 65536, kind) for kind in ("equal", "ints7")})
WHOLE = {f"whole_{k}_q{q}": (k, f"q{q}_b1_n65536") for k in ("bf16", "e4m3") for q in (1, 2)}


class Select:
    """`copies` logits buffers (rows, N_k) of one kind and the sides over them"""

    def __init__(self, name, dev):
        import torch
        import flash_attention_dlrs_amd as fa
        from flash_attention_dlrs_amd import _lib
        self.torch, self._lib = torch, _lib
        rows, N, kind = CASES[name]
        self.shape = dict(rows=rows, N_k=N, topk=TOPK, logits=kind)
        self.copies = max(2, math.ceil(300e6 / (4 * rows * N)))
        total = rows * self.copies
        if kind == "score":  # every copy a set of query positions of ONE score call over the same keys
            q = torch.randn(1, H_I, total, D_I, device=dev).to(torch.bfloat16)
            w = torch.randn(1, H_I, total, device=dev) * H_I ** -0.5
            k = torch.randn(1, N, D_I, device=dev).to(torch.bfloat16)
            lg = fa.mla_indexer_logits(q, w, k, None, dev, causal=False)[0]
        elif kind == "equal":
            lg = torch.full((total, N), 1.5, device=dev)
        else:
            lg = torch.randint(-3, 4, (total, N), device=dev).float()
        self.lg = lg.view(self.copies, 1, rows, N)
        self.idx = torch.empty(1, rows, TOPK, dtype=torch.int32, device=dev)
        self.auto = _lib.topk_num_splits(rows, N, TOPK)
        self.ws = torch.empty(max(_lib.topk_workspace_bytes(rows, 256), 16), dtype=torch.uint8, device=dev)
        self.mark = torch.zeros(1, device=dev)
        self.i = 0

    def _next(self):
        self.i = (self.i + 1) % self.copies
        return self.lg[self.i]

    def side(self, count):
        """count None: fa2_topk_indices; else fa2_topk_indices_split with that num_splits (0: the library's choice)"""
        if count is None:
            return lambda: self._lib.fa2_topk_indices(self._next(), self.idx, None, causal=False)
        return lambda: self._lib.fa2_topk_indices(self._next(), self.idx, None, causal=False, num_splits=count, workspace=self.ws)

    def torch_topk(self):
        def run():
            self.out = self.torch.topk(self._next(), TOPK, dim=-1)
        return run


def run_pass(name, args):
    """The traced child: each side warmed, then run back to back; the kernel trace holds the times."""
    import torch
    dev = torch.device("cuda:0")
    if name in WHOLE:
        k_dtype, case = WHOLE[name]
        c = IndexerCase(case, dev, k_dtype)
        ws = torch.empty(c._lib.topk_workspace_bytes(c.shape["B"] * c.shape["N_q"], 256), dtype=torch.uint8, device=dev)
        auto = c._lib.topk_num_splits(c.shape["B"] * c.shape["N_q"], c.shape["N_k"], TOPK)

        def split():
            k, ks = c._next()
            c._lib.fa2_mla_indexer_logits(c.q, c.w, k, ks, c.logits, c.lens, c.enum, c.k_enum, causal=True)
            c._lib.fa2_topk_indices(c.logits, c.indices, c.lens, causal=True, num_splits=0, workspace=ws)
        sides = [("fused", c.indexer("auto")), ("split", split), ("torch", c.torch_route())]
        info = dict(k_dtype=k_dtype, auto_count=auto, **c.shape)
    else:
        c = Select(name, dev)
        most = -(-c.shape["N_k"] // 1024)
        sides = [("s1", c.side(None))] + [(f"s{n}", c.side(n)) for n in COUNTS[1:] if n <= most] + [("auto", c.side(0)), ("torch", c.torch_topk())]
        info = dict(auto_count=c.auto, **c.shape)
    torch.cuda.synchronize()
    c.mark.fill_(0.0)  # the first marker: what lies before it is set-up
    for _, f in sides:
        timed(c, f, args.iters + 3)
    print(json.dumps(dict(case=name, order=[s for s, _ in sides], **info)))


def traced_child(out, name, args):
    os.makedirs(out, exist_ok=True)
    cmd = ["timeout", "-k", "10", str(args.child_timeout), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out,
           "--", sys.executable, os.path.abspath(__file__), "--iters", str(args.iters), "--pass-case", name]
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode != 0:  # a failed child ends the run: nothing more is started on the GPU
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
        sys.exit(p.returncode)
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def run_rocprof(names, args, fh):
    for name in names:
        out = os.path.join(args.rocprof, name)
        info = traced_child(out, name, args)
        order = info.pop("order")
        calls = call_times(out, len(order) * (args.iters + 3))
        sides = {}
        for pos, side in enumerate(order):
            mine = calls[pos * (args.iters + 3):(pos + 1) * (args.iters + 3)][3:]
            sides[side] = dict(spread([t for t, _, _ in mine]), calls=len(mine), kernels=sorted({k for _, _, ks in mine for k in ks}))
        base = sides[order[0]]
        over = {f"{s}_over_{order[0]}": round(v["avg_us"] / base["avg_us"], 4) for s, v in sides.items() if s != order[0]}
        overlap = {f"{s}_ranges_overlap": v["max_us"] >= base["min_us"] and base["max_us"] >= v["min_us"] for s, v in sides.items() if s != order[0]}
        emit(fh, kind="whole" if name in WHOLE else "select", **info, **over, **overlap, **sides)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(list(CASES) + list(WHOLE)))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rocprof", metavar="DIR", default=os.path.join(ROOT, "bench_out", "topk_select_traces"),
                    help="the traces of the rocprofv3 children go under DIR")
    ap.add_argument("--child-timeout", type=int, default=240)
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
