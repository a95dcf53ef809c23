#!/usr/bin/env python3
"""MLA decode timing (fa2_fwd_kvcache_mla: d = 576, d_v = 512, V = K[..., :512]), bf16, H_kv = 1; JSON lines appended to
profiles/mla/bench_mla_decode.jsonl.  --kv-dtype e4m3 / e5m2: the same shapes, protocol and sides over an fp8 latent cache
(fa2_fwd_kvcache_mla_fp8, the cache quantised by quantize_kv_cache with its per-sequence descale; sdpa on the dequantised bf16
tensors); every record carries kv_dtype, and kv_bytes, hbm_share and cache_gbps count the cache's own bytes per key (576 for fp8).  The protocol is benchmarks/bench_decode.py's: kernel times come from a
`rocprofv3 --kernel-trace --stats` child per shape (a fresh process, under its own `timeout -k 10`; the first non-zero status ends
the run), every side rotates over enough copies of the latent cache to exceed the 256 MiB last-level cache, and avg, min-max and
stddev are reported per call.

Sides of one child, each warmed (3 calls, not counted) and then run back to back:
  auto:    flash_attention_mla_decode_forward's launch, AUTO variant, auto num_splits (contiguous, or paged with --page-size 64:
           the cache scattered into a pool under a random permutation table);
  generic: the same launch, the VALU form forced, the same num_splits;
  sdpa:    torch scaled_dot_product_attention on the same absorbed tensors, contiguous only: K (B, 1, S, 576), V its first 512
           columns, and the H heads of a token as the query rows of that one KV head, Q (B, 1, H N_q, 576) -- the form that
           reads the latent cache once (no mask: the benchmark's calls have none).
The kernel trace is cut into the sides by dispatch order (split kernel plus combine per call; one kernel for num_splits = 1; the
rest after the last decode kernel is sdpa's).  hbm_share counts 1,152 B per visible key ONCE over the side's kernel time, as a
share of the 6.29 TB/s copy rate (cache_gbps: the same bytes over AUTO's time, in GB/s): a second row tile (128 heads, or 64 heads at N_q = 2) reads the keys again and is not counted.

--append: a decode step WITH its cache update (N_new = N_q rows per sequence at cache_seqlens = N_k - N_q, rotary_dim 64).  The fused
call (fa2_fwd_kvcache_mla_append) against what a caller does without it -- the torch restatement on the device (rotate k_pe,
concatenate, quantise, scatter through the table, rotate and concatenate Q) followed by the read-only decode launch -- alternated
call by call in ONE process and timed by device events around each call, --repeats runs per case; then the append launch alone
(fa2_kvcache_mla_append) with the bytes it must move, computed from the shapes, and bytes / s at its fastest rate (200 launches back to back without a host synchronisation).

Records:
  kind=append         --append: per case, the per-run avg / min / max / stddev of both sides, their ratio, the append launch alone;
  kind=kernels        one per shape and cache form: the sides' avg / min / max / stddev in microseconds, auto_over_generic;
  kind=sweep_kernels  --sweep: AUTO's variant under num_splits in SWEEP_SPLITS on the four SWEEP_CASES, one traced child per shape."""
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
OUT = os.path.join(ROOT, "profiles", "mla", "bench_mla_decode.jsonl")
HBM_COPY_RATE = 6.29e12  # bytes / s, measured copy rate of the MI355X
D, D_V = 576, 512
KV_DTYPES = ("bf16", "e4m3", "e5m2")

SHAPES = ((1, 8192), (1, 65536), (16, 4096), (64, 2048), (128, 4096))  # (B, N_k)
CASES = {f"h{H}_q{N_q}_b{B}_n{S}": (B, H, N_q, S) for H in (16, 128) for N_q in (1, 2) for B, S in SHAPES}
SWEEP_CASES = ("h128_q1_b1_n8192", "h128_q1_b1_n65536", "h128_q1_b16_n4096", "h16_q1_b1_n65536")
SWEEP_SPLITS = (1, 2, 4, 8, 16, 32, 64, 128)


def emit(fh, **kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if fh is not None:
        fh.write(line + "\n")
        fh.flush()


class Case:
    def __init__(self, name, dev, page_size=0, kv_dtype="bf16"):
        import torch
        import flash_attention_dlrs_amd as fa
        from flash_attention_dlrs_amd import _lib
        from flash_attention_dlrs_amd.flash_attention_torch import convert_triton_dtype
        self.torch, self._lib, self.dev = torch, _lib, dev
        B, H, N_q, S = CASES[name]
        self.shape = dict(B=B, H=H, N_q=N_q, N_k=S)
        self.fmt = {"bf16": None, "e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}[kv_dtype]
        self.kv_bytes = (1 if self.fmt else 2) * D * B * S
        self.copies = max(2, math.ceil(300e6 / self.kv_bytes))
        self.scale = D ** -0.5
        self.enum = convert_triton_dtype(torch.bfloat16)
        mk = lambda *s: (torch.randn(*s, device=dev) * 0.8).to(torch.bfloat16)  # noqa: E731
        self.Q = mk(B, H, N_q, D)
        self.KV = [mk(B, 1, S, D) for _ in range(self.copies)]
        self.KV16, self.descale, self.kv_enum = self.KV, None, self.enum  # KV16: what sdpa reads (fp8: the dequantised rows)
        if self.fmt:
            quant = [fa.quantize_kv_cache(t, self.fmt) for t in self.KV]
            self.KV, self.descale = [q[0] for q in quant], [q[1] for q in quant]
            self.KV16 = [fa.dequantize_kv_cache(k8, ds, torch.bfloat16) for k8, ds in quant]
            self.kv_enum = convert_triton_dtype(self.fmt)
        self.lens = torch.full((B,), S, dtype=torch.int32, device=dev)
        self.O = torch.empty(B, H, N_q, D_V, dtype=torch.bfloat16, device=dev)
        self.L = torch.empty(B, H, N_q, dtype=torch.bfloat16, device=dev)
        self.i = 0
        self.page_size, self.table = page_size, None
        if page_size:  # every copy scattered into a pool (num_blocks, 1, P, 576) under one random table
            mb = S // page_size
            perm = torch.randperm(B * mb, generator=torch.Generator().manual_seed(0)).to(dev)
            self.table = perm.view(B, mb).to(torch.int32)
            for k, t in enumerate(self.KV):  # (scattered as raw bytes or words: the fp8 dtypes have no indexed copy)
                raw = t.view(torch.uint8 if self.fmt else torch.int16).view(B * mb, 1, page_size, D)
                p = torch.empty_like(raw)
                p[perm] = raw
                self.KV[k] = p.view(t.dtype)

    def auto_splits(self):
        s = self.shape
        return self._lib.kvcache_mla_num_splits(s["B"], s["H"], 1, s["N_q"], s["N_k"], D, D_V, self.enum)

    def decode(self, variant, num_splits=0):
        """The library launch itself, outputs and workspace allocated once (what a serving loop does)."""
        s = self.shape
        n = num_splits or self.auto_splits()
        words = self._lib.kvcache_workspace_bytes(s["B"], s["H"], s["N_q"], D_V, n) // 4
        ws = self.torch.empty(max(words, 1), dtype=self.torch.float32, device=self.dev)

        def run():
            self.i = (self.i + 1) % self.copies
            kv = self.KV[self.i]
            if self.fmt:
                ds = self.descale[self.i]
                self._lib.fa2_fwd_kvcache_mla_fp8(self.Q, kv, kv[..., :D_V], self.O, self.L, self.lens, self.enum, self.kv_enum,
                                                  k_descale=ds, v_descale=ds, block_table=self.table, scale=self.scale, num_splits=n,
                                                  workspace=ws, variant=self._lib.KVCACHE_MLA_VARIANTS[variant])
                return
            self._lib.fa2_fwd_kvcache_mla(self.Q, kv, kv[..., :D_V], self.O, self.L, self.lens, self.enum, block_table=self.table,
                                          scale=self.scale, num_splits=n, workspace=ws, variant=self._lib.KVCACHE_MLA_VARIANTS[variant])
        return run

    def sdpa(self):
        F = self.torch.nn.functional

        def run():
            self.i = (self.i + 1) % self.copies
            kv = self.KV16[self.i]
            F.scaled_dot_product_attention(self.Q.view(self.Q.shape[0], 1, -1, D), kv, kv[..., :D_V], scale=self.scale)
        return run


def generic_iters(shape, iters):
    """the VALU form reads the keys once per query head: fewer calls where one takes tens of milliseconds"""
    return max(3, min(iters, int(2e8 / (shape["B"] * shape["H"] * shape["N_q"] * shape["N_k"]))))


def run_pass(name, args):
    """The traced child: each side warmed, then run back to back; the kernel trace holds the times."""
    import torch
    c = Case(name, torch.device("cuda:0"), args.page_size, args.kv_dtype)
    calls = {"auto": args.iters + 3, "generic": generic_iters(c.shape, args.iters) + 3}
    sides = [("auto", c.decode("auto")), ("generic", c.decode("generic"))]
    if not args.page_size and not args.no_sdpa:
        sides.append(("sdpa", c.sdpa()))
        calls["sdpa"] = generic_iters(c.shape, args.iters) + 3
    for side, f in sides:
        for _ in range(calls[side]):
            f()
        torch.cuda.synchronize()
    print(json.dumps(dict(case=name, calls=calls, kv_dtype=args.kv_dtype, kv_bytes=c.kv_bytes, num_splits=c.auto_splits(),
                          page_size=args.page_size, **c.shape)))


def run_sweep_pass(name, args):
    """The traced child of the split sweep: AUTO's variant alone, one split count after the other."""
    import torch
    c = Case(name, torch.device("cuda:0"), kv_dtype=args.kv_dtype)
    for n in SWEEP_SPLITS:
        f = c.decode("auto", n)
        for _ in range(args.iters + 3):
            f()
        torch.cuda.synchronize()
    print(json.dumps(dict(case=name, calls=args.iters + 3, kv_dtype=args.kv_dtype, auto_splits=c.auto_splits(), kv_bytes=c.kv_bytes,
                          **c.shape)))


def traced_child(out, extra, args):
    os.makedirs(out, exist_ok=True)
    cmd = ["timeout", "-k", "10", str(args.child_timeout), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out,
           "--", sys.executable, os.path.abspath(__file__), "--iters", str(args.iters), "--page-size", str(args.page_size), "--kv-dtype", args.kv_dtype] + \
        extra + \
        (["--no-sdpa"] if args.no_sdpa else [])
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode != 0:  # a failed child ends the run: nothing more is started on the GPU
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
        sys.exit(p.returncode)
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def trace_rows(out):
    trace = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
    return sorted(csv.DictReader(open(trace[0])), key=lambda r: int(r["Start_Timestamp"]))


def per_call(seg, per, calls, warm=3):
    """avg / min / max / stddev of the kernel time per call, the first `warm` calls (warm-up) left out"""
    us = [sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in seg[per * k:per * k + per]) / 1e3 for k in range(warm, calls)]
    avg = sum(us) / len(us)
    return dict(avg_us=round(avg, 2), min_us=round(min(us), 2), max_us=round(max(us), 2),
                stddev_us=round((sum((u - avg) ** 2 for u in us) / len(us)) ** 0.5, 2), calls=len(us),
                kernels=sorted({r["Kernel_Name"][:60] for r in seg}))


def sides_from_trace(out, info):
    rows = trace_rows(out)
    dec = [k for k, r in enumerate(rows) if "fa2_decode" in r["Kernel_Name"]]
    per = 1 if info["num_splits"] == 1 else 2
    na, ng = info["calls"]["auto"], info["calls"]["generic"]
    assert len(dec) == per * (na + ng), (len(dec), per, na, ng)
    fa = [rows[k] for k in dec]
    sides = {"auto": per_call(fa[:per * na], per, na), "generic": per_call(fa[per * na:], per, ng)}
    if "sdpa" in info["calls"]:
        # torch's first calls may launch kernels the later ones do not: the timed calls are cut from the END of the trace, by the
        # shortest period in which the kernel names of the last ns - 3 calls repeat
        rest, timed = rows[dec[-1] + 1:], info["calls"]["sdpa"] - 3
        names = [r["Kernel_Name"] for r in rest]
        per = next((p for p in range(1, len(names) // timed + 1)
                    if all(names[-k - 1] == names[-k - 1 - p] for k in range(p * (timed - 1)))), 0)
        if per:
            sides["sdpa"] = per_call(rest[-per * timed:], per, timed, warm=0)
    return sides


def run_rocprof(names, args, fh):
    for name in names:
        out = os.path.join(args.rocprof, name + (f"_p{args.page_size}" if args.page_size else "") +
                           ("" if args.kv_dtype == "bf16" else "_" + args.kv_dtype))
        info = traced_child(out, ["--pass-case", name], args)
        sides = sides_from_trace(out, info)
        a, g = sides["auto"], sides["generic"]
        emit(fh, kind="kernels", **{k: v for k, v in info.items() if k != "calls"},
             hbm_share=round(info["kv_bytes"] / (a["avg_us"] * 1e-6) / HBM_COPY_RATE, 3),
             cache_gbps=round(info["kv_bytes"] / (a["avg_us"] * 1e-6) / 1e9, 1),
             hbm_share_generic=round(info["kv_bytes"] / (g["avg_us"] * 1e-6) / HBM_COPY_RATE, 3),
             auto_over_generic=round(a["avg_us"] / g["avg_us"], 4), ranges_overlap=a["max_us"] >= g["min_us"], **sides)
        if args.sweep and name in SWEEP_CASES and not args.page_size:
            out = os.path.join(args.rocprof, name + "_sweep" + ("" if args.kv_dtype == "bf16" else "_" + args.kv_dtype))
            info = traced_child(out, ["--sweep-case", name], args)
            rows = [r for r in trace_rows(out) if "fa2_decode" in r["Kernel_Name"]]
            pos, calls = 0, info["calls"]
            for n in SWEEP_SPLITS:
                per = 1 if n == 1 else 2
                r = per_call(rows[pos:pos + per * calls], per, calls)
                pos += per * calls
                emit(fh, kind="sweep_kernels", case=name, kv_dtype=args.kv_dtype, num_splits=n, auto_splits=info["auto_splits"],
                     hbm_share=round(info["kv_bytes"] / (r["avg_us"] * 1e-6) / HBM_COPY_RATE, 3), **r)
            assert pos == len(rows)


class AppendCase(Case):
    """A decode step WITH its cache update (--append): N_new = N_q new rows per sequence at cache_seqlens = N_k - N_q, rotary_dim 64."""

    def __init__(self, name, dev, page_size=0, kv_dtype="bf16"):
        super().__init__(name, dev, page_size, kv_dtype)
        torch, s = self.torch, self.shape
        import flash_attention_dlrs_amd as fa
        self.fa = fa
        B, N = s["B"], s["N_q"]
        mk = lambda *sh: (torch.randn(*sh, device=dev) * 0.8).to(torch.bfloat16)  # noqa: E731
        self.c_new, self.pe_new = mk(B, 1, N, D_V), mk(B, 1, N, D - D_V)
        ang = torch.rand(s["N_k"], (D - D_V) // 2, device=dev, dtype=torch.float64) * 6.283
        self.cos, self.sin = ang.cos().to(torch.bfloat16), ang.sin().to(torch.bfloat16)
        self.lens = torch.full((B,), s["N_k"] - N, dtype=torch.int32, device=dev)
        self.out = torch.empty_like(self.lens)
        self.q_rot = torch.empty_like(self.Q)
        self.n = self.auto_splits()
        self.ws = torch.empty(max(self._lib.kvcache_workspace_bytes(B, s["H"], N, D_V, self.n) // 4, 1), dtype=torch.float32, device=dev)
        # the bytes the append launch alone must move: the two sources, the cache rows, the table rows of each position, the lengths
        csz = 1 if self.fmt else 2
        self.append_bytes = B * N * (2 * D + csz * D + 2 * (D - D_V)) + 8 * B

    def _next(self):
        self.i = (self.i + 1) % self.copies
        return self.KV[self.i], (self.descale[self.i] if self.fmt else None)

    def fused(self):
        kv, ds = self._next()
        self._lib.fa2_fwd_kvcache_mla_append(self.Q, kv, self.O, self.L, self.c_new, self.pe_new, self.lens, self.out, self.enum,
                                             self.kv_enum, block_table=self.table, kv_descale=ds, rotary_cos=self.cos,
                                             rotary_sin=self.sin, q_rot=self.q_rot, scale=self.scale, num_splits=self.n,
                                             workspace=self.ws)

    def append_alone(self):
        kv, ds = self._next()
        self._lib.fa2_kvcache_mla_append(kv, self.c_new, self.pe_new, self.lens, self.out, self.enum, self.kv_enum,
                                         block_table=self.table, kv_descale=ds, rotary_cos=self.cos, rotary_sin=self.sin)

    def torch_then_decode(self):
        """What a caller has to do without the append: rotate, concatenate, quantise, scatter through the table, rotate and
        concatenate Q in torch on the device, then the read-only decode launch."""
        torch, fa, s = self.torch, self.fa, self.shape
        kv, ds = self._next()
        B, N, P = s["B"], s["N_q"], self.page_size
        idx = self.lens.long()[:, None] + torch.arange(N, device=self.dev)[None, :]  # (B, N) key indices
        row = torch.cat([self.c_new, fa.apply_rotary(self.pe_new, self.cos, self.sin, idx[:, None, :])], dim=-1)
        if self.fmt:
            top = torch.finfo(self.fmt).max
            row = (row.float() / ds[:, :, None, None]).clamp(-top, top).to(self.fmt)
        raw, rows = kv.view(torch.uint8 if self.fmt else torch.int16), row.view(torch.uint8 if self.fmt else torch.int16)[:, 0]
        if P:
            raw[self.table.long().gather(1, idx // P), 0, idx % P] = rows
        else:
            raw[torch.arange(B, device=self.dev)[:, None], 0, idx] = rows
        q = torch.cat([self.Q[..., :D_V], fa.apply_rotary(self.Q[..., D_V:], self.cos, self.sin, self.lens.long()[:, None, None])], dim=-1)
        new_lens = self.lens + N
        if self.fmt:
            self._lib.fa2_fwd_kvcache_mla_fp8(q, kv, kv[..., :D_V], self.O, self.L, new_lens, self.enum, self.kv_enum, k_descale=ds,
                                              v_descale=ds, block_table=self.table, scale=self.scale, num_splits=self.n, workspace=self.ws)
        else:
            self._lib.fa2_fwd_kvcache_mla(q, kv, kv[..., :D_V], self.O, self.L, new_lens, self.enum, block_table=self.table,
                                          scale=self.scale, num_splits=self.n, workspace=self.ws)


def stats_us(us):
    avg = sum(us) / len(us)
    return dict(avg_us=round(avg, 2), min_us=round(min(us), 2), max_us=round(max(us), 2),
                stddev_us=round((sum((u - avg) ** 2 for u in us) / len(us)) ** 0.5, 2), calls=len(us))


def run_append(names, args, fh):
    """--append: the fused step against the torch restatement plus the decode launch, alternated call by call in this one process
    and timed by device events around each call (both sides are several launches, so this is the time a stream spends on a step,
    launch gaps included); then the append launch alone, with its bytes.  Repeated --repeats times: the spread of the averages."""
    import torch
    dev = torch.device("cuda:0")
    for name in names:
        c = AppendCase(name, dev, args.page_size, args.kv_dtype)
        sides = (("fused", c.fused), ("torch_then_decode", c.torch_then_decode))
        runs = {k: [] for k, _ in sides}
        alone = []
        for _ in range(args.repeats):
            times = {k: [] for k, _ in sides}
            for it in range(args.iters + 3):
                for k, f in sides:
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    f()
                    b.record()
                    b.synchronize()
                    if it >= 3:
                        times[k].append(a.elapsed_time(b) * 1e3)
            for k in times:
                runs[k].append(stats_us(times[k]))
            t = []
            for it in range(args.iters + 3):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                c.append_alone()
                b.record()
                b.synchronize()
                if it >= 3:
                    t.append(a.elapsed_time(b) * 1e3)
            alone.append(stats_us(t))
            # ... and back to back, no host synchronisation between the calls: the stream's time per launch
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(200):
                c.append_alone()
            b.record()
            b.synchronize()
            alone[-1]["back_to_back_us"] = round(a.elapsed_time(b) * 1e3 / 200, 3)
        f_avg, p_avg = [r["avg_us"] for r in runs["fused"]], [r["avg_us"] for r in runs["torch_then_decode"]]
        a_min = min(r["back_to_back_us"] for r in alone)
        emit(fh, kind="append", case=name, kv_dtype=args.kv_dtype, page_size=args.page_size, num_splits=c.n, **c.shape,
             fused=runs["fused"], torch_then_decode=runs["torch_then_decode"],
             fused_over_parent=[round(f / p, 4) for f, p in zip(f_avg, p_avg)],
             ranges_overlap=max(f_avg) >= min(p_avg), append_alone=alone, append_bytes=c.append_bytes,
             append_gbps_at_min=round(c.append_bytes / (a_min * 1e-6) / 1e9, 3),
             append_hbm_share_at_min=round(c.append_bytes / (a_min * 1e-6) / HBM_COPY_RATE, 6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--sweep", action="store_true", help="also time num_splits in %s on %s" % (SWEEP_SPLITS, SWEEP_CASES))
    ap.add_argument("--no-sdpa", action="store_true")
    ap.add_argument("--rocprof", metavar="DIR", default=os.path.join(ROOT, "bench_out", "mla_traces"),
                    help="the traces of the rocprofv3 children go under DIR")
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--page-size", type=int, default=0, metavar="N", help="the paged cache at N-key pages (64) in the contiguous one's place")
    ap.add_argument("--kv-dtype", choices=KV_DTYPES, default="bf16", help="the latent cache's storage: bf16, or fp8 with its descale")
    ap.add_argument("--append", action="store_true",
                    help="time the fused append + decode step against the torch restatement + decode, and the append launch alone")
    ap.add_argument("--repeats", type=int, default=3, help="--append: runs per case, for the spread of the averages")
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
        if args.append:
            return run_append(args.cases.split(","), args, fh)
        run_rocprof(args.cases.split(","), args, fh)


if __name__ == "__main__":
    main()
