#!/usr/bin/env python3
"""Sparse MLA decode timing (fa2_fwd_kvcache_mla_sparse: d = 576, d_v = 512, per-query lists of topk = 2048 keys), bf16 Q over a bf16
or e4m3 latent cache, H_kv = 1; JSON lines appended to profiles/mla/bench_mla_sparse.jsonl.  The protocol is
benchmarks/bench_mla_decode.py's: kernel times come from a `rocprofv3 --kernel-trace --stats` child per shape (a fresh process, under
its own `timeout -k 10`; the first non-zero status ends the run), every side rotates over enough copies of the latent cache to exceed
the 256 MiB last-level cache, each side is warmed (3 calls, not counted) and then run back to back, and avg, min-max and stddev are
reported per call.  A one-element fill launched after every call marks the call boundaries in the trace; it is not counted.

Lists: for every (b, qi) topk distinct positions of [0, N_k), in random order (torch.topk's lists are not sorted by position), one list
for the KV head; --sorted puts each list in ascending position, as fa2_topk_indices emits it.  Sides of one child:
  auto          the sparse launch, AUTO variant, auto num_splits;
  generic       the same launch, the VALU form forced, the same num_splits;
  gather_dense  the only earlier route: torch index_select of the listed rows into a temporary (B N_q, 1, topk, 576) cache, then the
                dense MLA launch over it (B N_q sequences of one query, its own auto num_splits); both kernels counted, the flat
                int64 row numbers prepared outside the timed calls;
  dense_topk    the dense MLA launch alone over topk CONTIGUOUS keys per (b, qi), windows of the rotating caches (from HBM, as the
                lists' rows are): what the same arithmetic costs without per-row addressing;
  dense_all     the dense MLA launch over all N_k keys: what the sparsity saves.

Records:
  kind=kernels        one per shape and cache dtype: the sides' avg / min / max / stddev in microseconds, the ratios of AUTO to each
                      other side, and whether AUTO's min-max range overlaps the gather route's and the VALU form's;
  kind=sweep_kernels  --sweep: AUTO's variant under num_splits in SWEEP_SPLITS on SWEEP_CASES, one traced child per shape."""
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
OUT = os.path.join(ROOT, "profiles", "mla", "bench_mla_sparse.jsonl")
D, D_V, TOPK = 576, 512, 2048
KV_DTYPES = ("bf16", "e4m3")

SHAPES = ((1, 65536), (16, 16384), (128, 8192))  # (B, N_k)
CASES = {f"h{H}_q{N_q}_b{B}_n{S}": (B, H, N_q, S) for H in (16, 128) for N_q in (1, 2) for B, S in SHAPES}
CASES["prefill_h128_q1024_b1_n16384"] = (1, 128, 1024, 16384)  # one sparse prefill chunk
SWEEP_CASES = ("h128_q1_b1_n65536", "h16_q1_b1_n65536", "h128_q1_b16_n16384", "h16_q2_b16_n16384", "h128_q2_b128_n8192")
SWEEP_SPLITS = (1, 2, 4, 8, 16, 32)
MARK = "FillFunctor"


def emit(fh, **kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if fh is not None:
        fh.write(line + "\n")
        fh.flush()


class Case:
    def __init__(self, name, dev, kv_dtype="bf16", sort_lists=False):
        import torch
        import flash_attention_dlrs_amd as fa
        from flash_attention_dlrs_amd import _lib
        from flash_attention_dlrs_amd.flash_attention_torch import convert_triton_dtype
        self.torch, self._lib, self.dev = torch, _lib, dev
        B, H, N_q, S = CASES[name]
        self.shape = dict(B=B, H=H, N_q=N_q, N_k=S, topk=TOPK)
        self.fmt = {"bf16": None, "e4m3": torch.float8_e4m3fn}[kv_dtype]
        self.copies = max(2, math.ceil(300e6 / ((1 if self.fmt else 2) * D * B * S)))
        self.scale = D ** -0.5
        self.enum = convert_triton_dtype(torch.bfloat16)
        mk = lambda *s: (torch.randn(*s, device=dev) * 0.8).to(torch.bfloat16)  # noqa: E731
        self.Q = mk(B, H, N_q, D)
        self.Q1 = self.Q.permute(0, 2, 1, 3).reshape(B * N_q, H, 1, D).contiguous()  # every (b, qi) a sequence of one query
        self.KV = [mk(B, 1, S, D) for _ in range(self.copies)]
        self.descale, self.kv_enum = None, self.enum
        if self.fmt:
            quant = [fa.quantize_kv_cache(t, self.fmt) for t in self.KV]
            self.KV, self.descale = [q[0] for q in quant], [q[1] for q in quant]
            self.kv_enum = convert_triton_dtype(self.fmt)
        g = torch.Generator(device=dev).manual_seed(0)
        self.idx = torch.stack([torch.rand(N_q, S, device=dev, generator=g).argsort(-1)[:, :TOPK] for _ in range(B)]).to(torch.int32)
        if sort_lists:  # --sorted: what an indexer that emits its lists in ascending key position hands over
            self.idx = self.idx.sort(-1).values
        self.flat = (self.idx.long() + torch.arange(B, device=dev).view(B, 1, 1) * S).view(-1)  # row numbers of the (B S, 576) cache
        self.lens = torch.full((B,), S, dtype=torch.int32, device=dev)
        self.lens1 = torch.full((B * N_q,), TOPK, dtype=torch.int32, device=dev)
        self.O = torch.empty(B, H, N_q, D_V, dtype=torch.bfloat16, device=dev)
        self.L = torch.empty(B, H, N_q, dtype=torch.bfloat16, device=dev)
        self.O1 = torch.empty(B * N_q, H, 1, D_V, dtype=torch.bfloat16, device=dev)
        self.L1 = torch.empty(B * N_q, H, 1, dtype=torch.bfloat16, device=dev)
        self.tmp = torch.empty(B * N_q, 1, TOPK, D, dtype=self.KV[0].dtype, device=dev)
        # dense_topk: (b, qi) reads the keys [qi step, qi step + topk) of sequence b; one stride over b N_q + qi, windows inside a sequence
        self.step = S // N_q if B > 1 else min(S // N_q, (S - TOPK) // max(N_q - 1, 1))
        assert (N_q - 1) * self.step + TOPK <= S
        self.mark = torch.zeros(1, device=dev)
        self.i = 0

    def _next(self):
        self.i = (self.i + 1) % self.copies
        return self.KV[self.i], (self.descale[self.i] if self.fmt else None)

    def sparse_splits(self):
        s = self.shape
        return self._lib.kvcache_mla_sparse_num_splits(s["B"], s["H"], 1, s["N_q"], TOPK, D, D_V, self.enum)

    def _ws(self, rows, n):
        return self.torch.empty(max(4 * n * rows * (D_V + 1) // 4, 1), dtype=self.torch.float32, device=self.dev)

    def sparse(self, variant, num_splits=0):
        s = self.shape
        n = num_splits or self.sparse_splits()
        ws = self._ws(s["B"] * s["H"] * s["N_q"], n)
        idx = self.idx.unsqueeze(1)

        def run():
            kv, ds = self._next()
            self._lib.fa2_fwd_kvcache_mla_sparse(self.Q, kv, kv[..., :D_V], self.O, self.L, idx, self.lens, self.enum, self.kv_enum,
                                                 k_descale=ds, v_descale=ds, scale=self.scale, num_splits=n, workspace=ws,
                                                 variant=self._lib.KVCACHE_MLA_VARIANTS[variant])
        return run

    def _dense(self, Q, kv, ds, O, L, lens, n, ws):
        if self.fmt:
            self._lib.fa2_fwd_kvcache_mla_fp8(Q, kv, kv[..., :D_V], O, L, lens, self.enum, self.kv_enum, k_descale=ds, v_descale=ds,
                                              scale=self.scale, num_splits=n, workspace=ws)
        else:
            self._lib.fa2_fwd_kvcache_mla(Q, kv, kv[..., :D_V], O, L, lens, self.enum, scale=self.scale, num_splits=n, workspace=ws)

    def dense1_splits(self):
        s = self.shape
        return self._lib.kvcache_mla_num_splits(s["B"] * s["N_q"], s["H"], 1, 1, TOPK, D, D_V, self.enum)

    def gather_dense(self):
        s = self.shape
        n = self.dense1_splits()
        ws = self._ws(s["B"] * s["H"] * s["N_q"], n)
        raw = self.torch.uint8 if self.fmt else self.torch.int16  # (gathered as raw bytes or words: the fp8 dtypes have no indexed copy)
        tmp2 = self.tmp.view(raw).view(-1, D)
        dsq = [None if d is None else d.repeat_interleave(s["N_q"], 0) for d in (self.descale or [None] * self.copies)]

        def run():
            kv, _ = self._next()
            self.torch.index_select(kv.view(raw).view(-1, D), 0, self.flat, out=tmp2)
            self._dense(self.Q1, self.tmp, dsq[self.i], self.O1, self.L1, self.lens1, n, ws)
        return run

    def dense_topk(self):
        s = self.shape
        n = self.dense1_splits()
        ws = self._ws(s["B"] * s["H"] * s["N_q"], n)
        dsq = [None if d is None else d.repeat_interleave(s["N_q"], 0) for d in (self.descale or [None] * self.copies)]

        def run():  # a strided view, no copy: (b, qi) is sequence b N_q + qi of the launch
            kv, _ = self._next()
            win = kv.as_strided((s["B"] * s["N_q"], 1, TOPK, D), (self.step * D, 0, D, 1))
            self._dense(self.Q1, win, dsq[self.i], self.O1, self.L1, self.lens1, n, ws)
        return run

    def dense_all(self):
        s = self.shape
        n = self._lib.kvcache_mla_num_splits(s["B"], s["H"], 1, s["N_q"], s["N_k"], D, D_V, self.enum)
        ws = self._ws(s["B"] * s["H"] * s["N_q"], n)

        def run():
            kv, ds = self._next()
            self._dense(self.Q, kv, ds, self.O, self.L, self.lens, n, ws)
        return run


def side_iters(side, shape, iters):
    """the VALU form reads a list once per 16 heads on the vector units, the dense call over all keys reads N_k / topk times the rows:
    fewer calls where one takes tens of milliseconds"""
    work = shape["B"] * shape["N_q"] * shape["H"] * (shape["N_k"] if side == "dense_all" else TOPK)
    if side == "generic":
        return max(3, min(iters, int(4e8 / work)))
    return max(3, min(iters, int(4e10 / work)))


def timed(c, f, calls):
    for _ in range(calls):
        f()
        c.mark.fill_(1.0)
    c.torch.cuda.synchronize()


def run_pass(name, args):
    """The traced child: each side warmed, then run back to back; the kernel trace holds the times."""
    import torch
    c = Case(name, torch.device("cuda:0"), args.kv_dtype, args.sorted)
    torch.cuda.synchronize()
    c.mark.fill_(0.0)  # the first marker: what lies before it is set-up
    sides = [("auto", c.sparse("auto")), ("generic", c.sparse("generic")), ("gather_dense", c.gather_dense()),
             ("dense_topk", c.dense_topk()), ("dense_all", c.dense_all())]
    calls = {}
    for side, f in sides:
        calls[side] = side_iters(side, c.shape, args.iters) + 3
        timed(c, f, calls[side])
    print(json.dumps(dict(case=name, calls=calls, order=[s for s, _ in sides], kv_dtype=args.kv_dtype, lists="sorted" if args.sorted else "random",
                          num_splits=c.sparse_splits(),
                          dense_topk_splits=c.dense1_splits(), **c.shape)))


def run_sweep_pass(name, args):
    """The traced child of the split sweep: AUTO's variant alone, one split count after the other."""
    import torch
    c = Case(name, torch.device("cuda:0"), args.kv_dtype)
    torch.cuda.synchronize()
    c.mark.fill_(0.0)
    for n in SWEEP_SPLITS:
        timed(c, c.sparse("auto", n), args.iters + 3)
    print(json.dumps(dict(case=name, calls=args.iters + 3, kv_dtype=args.kv_dtype, auto_splits=c.sparse_splits(), **c.shape)))


def traced_child(out, extra, args):
    os.makedirs(out, exist_ok=True)
    cmd = ["timeout", "-k", "10", str(args.child_timeout), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out,
           "--", sys.executable, os.path.abspath(__file__), "--iters", str(args.iters), "--kv-dtype", args.kv_dtype] + (["--sorted"] if args.sorted else []) + extra
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode != 0:  # a failed child ends the run: nothing more is started on the GPU
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
        sys.exit(p.returncode)
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def call_times(out, total):
    """the kernel time of each of the last `total` calls, in microseconds, and the kernel names of each: the trace cut at the marks (the
    set-up may fill tensors of its own: the timed calls are the segments between the last total + 1 marks)"""
    trace = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
    rows = sorted(csv.DictReader(open(trace[0])), key=lambda r: int(r["Start_Timestamp"]))
    marks = [k for k, r in enumerate(rows) if MARK in r["Kernel_Name"]][-(total + 1):]
    assert len(marks) == total + 1 and marks[-1] == len(rows) - 1, (len(marks), total, marks[-1], len(rows))
    calls = []
    for lo, hi in zip(marks, marks[1:]):
        seg = rows[lo + 1:hi]
        assert seg, "two marks with no kernel between them"
        calls.append((sum(int(x["End_Timestamp"]) - int(x["Start_Timestamp"]) for x in seg) / 1e3, sorted({x["Kernel_Name"][:60] for x in seg})))
    return calls


def stats(calls, warm=3):
    us = [t for t, _ in calls[warm:]]
    avg = sum(us) / len(us)
    return dict(avg_us=round(avg, 2), min_us=round(min(us), 2), max_us=round(max(us), 2),
                stddev_us=round((sum((u - avg) ** 2 for u in us) / len(us)) ** 0.5, 2), calls=len(us),
                kernels=sorted({k for _, ks in calls for k in ks}))


def run_rocprof(names, args, fh):
    for name in names:
        out = os.path.join(args.rocprof, name + "_" + args.kv_dtype)
        info = traced_child(out, ["--pass-case", name], args)
        calls = call_times(out, sum(info["calls"].values()))
        sides, pos = {}, 0
        for side in info["order"]:
            sides[side] = stats(calls[pos:pos + info["calls"][side]])
            pos += info["calls"][side]
        a = sides["auto"]
        emit(fh, kind="kernels", **{k: v for k, v in info.items() if k not in ("calls", "order")},
             auto_over_gather_dense=round(a["avg_us"] / sides["gather_dense"]["avg_us"], 4),
             gather_ranges_overlap=a["max_us"] >= sides["gather_dense"]["min_us"],
             auto_over_generic=round(a["avg_us"] / sides["generic"]["avg_us"], 4),
             generic_ranges_overlap=a["max_us"] >= sides["generic"]["min_us"],
             auto_over_dense_topk=round(a["avg_us"] / sides["dense_topk"]["avg_us"], 4),
             auto_over_dense_all=round(a["avg_us"] / sides["dense_all"]["avg_us"], 4), **sides)
        if args.sweep and name in SWEEP_CASES:
            out = os.path.join(args.rocprof, name + "_sweep_" + args.kv_dtype)
            info = traced_child(out, ["--sweep-case", name], args)
            per = info["calls"]
            calls = call_times(out, per * len(SWEEP_SPLITS))
            for k, n in enumerate(SWEEP_SPLITS):
                emit(fh, kind="sweep_kernels", case=name, kv_dtype=args.kv_dtype, num_splits=n, auto_splits=info["auto_splits"],
                     **stats(calls[k * per:(k + 1) * per]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--sweep", action="store_true", help="also time num_splits in %s on %s" % (SWEEP_SPLITS, SWEEP_CASES))
    ap.add_argument("--rocprof", metavar="DIR", default=os.path.join(ROOT, "bench_out", "mla_sparse_traces"),
                    help="the traces of the rocprofv3 children go under DIR")
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--kv-dtype", choices=KV_DTYPES, default="bf16", help="the latent cache's storage: bf16, or e4m3 with its descale")
    ap.add_argument("--sorted", action="store_true", help="every list in ascending key position (records carry lists=sorted)")
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
