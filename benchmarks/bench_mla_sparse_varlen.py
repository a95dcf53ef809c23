#!/usr/bin/env python3
"""Packed (ragged) sparse MLA step timing: the pair indexer + sparse attention (fa2_mla_indexer_topk_varlen into
fa2_fwd_kvcache_mla_sparse_varlen), bf16, H = 128, H_kv = 1, topk = 2,048, the indexer at H_I = 64 / d_I = 128; JSON lines appended to
profiles/mla/bench_mla_sparse_varlen.jsonl.  The protocol is benchmarks/bench_mla_sparse.py's: kernel times come from a `rocprofv3
--kernel-trace --stats` child per shape (a fresh process, under its own `timeout -k 10`; the first non-zero status ends the run), every
side rotates over copies of the latent cache and the index-key cache that together exceed the 256 MiB last-level cache, each side is
warmed (3 calls, not counted) and then run back to back, and avg, min-max and stddev are reported per call.  A one-element fill
launched after every call marks the call boundaries in the trace; it is not counted.

Shapes (every sequence holds N_k keys, the queries its last positions):
  chunk256_dec63   a 256-token prefill chunk beside 63 one-token decodes: B = 64, total_q = 319, max_seqlen_q = 256;
  uniform_q1_b64   a uniform one-token batch: B = 64, total_q = 64.

Sides of one child, each the pair of calls (score + selection kernels, then the sparse kernel and its combine):
  packed      the packed calls over cu_seqlens_q;
  padded      the fixed calls on a rectangular (B, max_seqlen_q) batch, every sequence padded to the longest chunk;
  per_count   one pair of fixed calls per distinct query count (the chunk alone, then the 63 decodes): what an engine does today
              without padding.  On the uniform batch it is the fixed call itself, and so is `padded`.

Records: kind=kernels, one per shape: the sides' avg / min / max / stddev in microseconds, each side's indexer and attention share,
packed over the other two, and whether packed's min-max range touches theirs."""
import argparse
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_mla_sparse import call_times, emit, stats  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "mla", "bench_mla_sparse_varlen.jsonl")
D, D_V, TOPK, H, H_I, D_I = 576, 512, 2048, 128, 64, 128
CASES = {"chunk256_dec63": ([256] + [1] * 63, 8192), "uniform_q1_b64": ([1] * 64, 8192)}  # (query counts, N_k)


class Case:
    def __init__(self, name, dev):
        import torch
        from flash_attention_dlrs_amd import _lib
        from flash_attention_dlrs_amd.flash_attention_torch import convert_triton_dtype
        self.torch, self._lib, self.dev = torch, _lib, dev
        counts, S = CASES[name]
        B, total, max_q = len(counts), sum(counts), max(counts)
        self.counts, self.B, self.S, self.total, self.max_q = counts, B, S, total, max_q
        self.shape = dict(B=B, H=H, total_q=total, max_seqlen_q=max_q, N_k=S, topk=TOPK, H_I=H_I, d_I=D_I)
        self.copies = max(2, math.ceil(300e6 / (2 * (D + D_I) * B * S)))
        self.scale = D ** -0.5
        self.enum = convert_triton_dtype(torch.bfloat16)
        bf = torch.bfloat16
        mk = lambda *s: (torch.randn(*s, device=dev) * 0.8).to(bf)  # noqa: E731
        self.KV = [mk(B, 1, S, D) for _ in range(self.copies)]
        self.KI = [mk(B, S, D_I) for _ in range(self.copies)]
        self.lens = torch.full((B,), S, dtype=torch.int32, device=dev)
        starts = [sum(counts[:b]) for b in range(B + 1)]
        self.cu = torch.tensor(starts, dtype=torch.int32, device=dev)
        # packed operands
        self.Q, self.qi = mk(total, H, D), mk(total, H_I, D_I)
        self.w = torch.randn(total, H_I, device=dev) * H_I ** -0.5
        self.O, self.L = torch.empty(total, H, D_V, dtype=bf, device=dev), torch.empty(H, total, dtype=bf, device=dev)
        self.lg, self.ix = torch.empty(total, S, device=dev), torch.empty(total, TOPK, dtype=torch.int32, device=dev)
        # the groups of equal query count, each a contiguous run of sequences (the chunk first): (first sequence, sequences, count)
        self.groups = []
        for b, n in enumerate(counts):
            if self.groups and self.groups[-1][2] == n:
                self.groups[-1][1] += 1
            else:
                self.groups.append([b, 1, n])
        self.fixed = {(nb, n): self._fixed_operands(nb, n) for _, nb, n in self.groups}
        if (B, max_q) not in self.fixed:
            self.fixed[(B, max_q)] = self._fixed_operands(B, max_q)
        self.mark = torch.zeros(1, device=dev)
        self.i = 0

    def _fixed_operands(self, nb, n):
        """the rectangular operands of a fixed pair on nb sequences of n queries: Q, q_idx, weights, O, L, logits, indices"""
        t, bf = self.torch, self.torch.bfloat16
        mk = lambda *s: (t.randn(*s, device=self.dev) * 0.8).to(bf)  # noqa: E731
        return dict(Q=mk(nb, H, n, D), qi=mk(nb, H_I, n, D_I), w=t.randn(nb, H_I, n, device=self.dev) * H_I ** -0.5,
                    O=t.empty(nb, H, n, D_V, dtype=bf, device=self.dev), L=t.empty(nb, H, n, dtype=bf, device=self.dev),
                    lg=t.empty(nb, n, self.S, device=self.dev), ix=t.empty(nb, n, TOPK, dtype=t.int32, device=self.dev))

    def _next(self):
        self.i = (self.i + 1) % self.copies
        return self.KV[self.i], self.KI[self.i]

    def _ws(self, rows, n):
        return self.torch.empty(max(n * rows * (D_V + 1), 1), dtype=self.torch.float32, device=self.dev)

    def packed_splits(self):
        return self._lib.kvcache_mla_sparse_varlen_num_splits(self.total, H, 1, TOPK, D, D_V, self.enum)

    def packed(self):
        n = self.packed_splits()
        ws = self._ws(self.total * H, n)

        def run():
            kv, ki = self._next()
            self._lib.fa2_mla_indexer_topk_varlen(self.qi, self.w, ki, None, self.lg, self.ix, self.cu, self.max_q, self.lens, self.enum, self.enum)
            self._lib.fa2_fwd_kvcache_mla_sparse_varlen(self.Q, kv, kv[..., :D_V], self.O, self.L, self.ix.unsqueeze(1), self.cu, self.max_q,
                                                        self.lens, self.enum, self.enum, scale=self.scale, num_splits=n, workspace=ws)
        return run

    def _fixed_pair(self, first, nb, n):
        ops = self.fixed[(nb, n)]
        ns = self._lib.kvcache_mla_sparse_num_splits(nb, H, 1, n, TOPK, D, D_V, self.enum)
        ws = self._ws(nb * H * n, ns)
        lens = self.lens[first:first + nb]

        def run(kv, ki):
            self._lib.fa2_mla_indexer_topk(ops["qi"], ops["w"], ki[first:first + nb], None, ops["lg"], ops["ix"], lens, self.enum, self.enum)
            kvb = kv[first:first + nb]
            self._lib.fa2_fwd_kvcache_mla_sparse(ops["Q"], kvb, kvb[..., :D_V], ops["O"], ops["L"], ops["ix"].unsqueeze(1), lens, self.enum,
                                                 self.enum, scale=self.scale, num_splits=ns, workspace=ws)
        return run, ns

    def padded(self):
        pair, _ = self._fixed_pair(0, self.B, self.max_q)

        def run():
            pair(*self._next())
        return run

    def per_count(self):
        pairs = [self._fixed_pair(first, nb, n)[0] for first, nb, n in self.groups]

        def run():
            kv, ki = self._next()
            for pair in pairs:
                pair(kv, ki)
        return run


def timed(c, f, calls):
    for _ in range(calls):
        f()
        c.mark.fill_(1.0)
    c.torch.cuda.synchronize()


def run_pass(name, args):
    """The traced child: each side warmed, then run back to back; the kernel trace holds the times."""
    import torch
    c = Case(name, torch.device("cuda:0"))
    torch.cuda.synchronize()
    c.mark.fill_(0.0)  # the first marker: what lies before it is set-up
    sides = [("packed", c.packed()), ("padded", c.padded()), ("per_count", c.per_count())]
    calls = {}
    for side, f in sides:
        # (the padded side of the ragged shape runs B * max_seqlen_q positions: fewer calls where one takes tens of milliseconds)
        calls[side] = (max(3, args.iters // 4) if side == "padded" and c.B * c.max_q > 4 * c.total else args.iters) + 3
        timed(c, f, calls[side])
    print(json.dumps(dict(case=name, calls=calls, order=[s for s, _ in sides], num_splits=c.packed_splits(),
                          groups=[[nb, n] for _, nb, n in c.groups], **c.shape)))


def traced_child(out, extra, args):
    os.makedirs(out, exist_ok=True)
    cmd = ["timeout", "-k", "10", str(args.child_timeout), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out,
           "--", sys.executable, os.path.abspath(__file__), "--iters", str(args.iters)] + extra
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode != 0:  # a failed child ends the run: nothing more is started on the GPU
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
        sys.exit(p.returncode)
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def shares(calls, warm=3):
    """the average microseconds per call of the indexer's kernels (scores and selection) and of the attention's (sparse and combine)"""
    idx = att = 0.0
    for _, _, per_kernel in calls[warm:]:
        for k, us in per_kernel.items():
            if "indexer" in k or "topk_indices" in k:
                idx += us
            else:
                att += us
    n = max(len(calls) - warm, 1)
    return dict(indexer_us=round(idx / n, 2), attention_us=round(att / n, 2))


def call_kernels(out, total):
    """call_times with the per-kernel microseconds of each call beside it"""
    import csv
    import glob
    trace = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
    rows = sorted(csv.DictReader(open(trace[0])), key=lambda r: int(r["Start_Timestamp"]))
    marks = [k for k, r in enumerate(rows) if "FillFunctor" in r["Kernel_Name"]][-(total + 1):]
    out_calls = []
    for (t, names), lo, hi in zip(call_times(out, total), marks, marks[1:]):
        per = {}
        for x in rows[lo + 1:hi]:
            per[x["Kernel_Name"][:60]] = per.get(x["Kernel_Name"][:60], 0.0) + (int(x["End_Timestamp"]) - int(x["Start_Timestamp"])) / 1e3
        out_calls.append((t, names, per))
    return out_calls


def run_rocprof(names, args, fh):
    for name in names:
        out = os.path.join(args.rocprof, name)
        info = traced_child(out, ["--pass-case", name], args)
        calls = call_kernels(out, sum(info["calls"].values()))
        sides, pos = {}, 0
        for side in info["order"]:
            seg = calls[pos:pos + info["calls"][side]]
            sides[side] = dict(stats([(t, ks) for t, ks, _ in seg]), **shares(seg))
            pos += info["calls"][side]
        p = sides["packed"]
        emit(fh, kind="kernels", **{k: v for k, v in info.items() if k not in ("calls", "order")},
             packed_over_padded=round(p["avg_us"] / sides["padded"]["avg_us"], 4),
             padded_ranges_touch=p["max_us"] >= sides["padded"]["min_us"] and sides["padded"]["max_us"] >= p["min_us"],
             packed_over_per_count=round(p["avg_us"] / sides["per_count"]["avg_us"], 4),
             per_count_ranges_touch=p["max_us"] >= sides["per_count"]["min_us"] and sides["per_count"]["max_us"] >= p["min_us"], **sides)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rocprof", metavar="DIR", default=os.path.join(ROOT, "bench_out", "mla_sparse_varlen_traces"),
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
