#!/usr/bin/env python3
"""Timing of the quantising cache writers (fa2_kvcache_mla_append_ds, fa2_mla_indexer_append and their packed forms) beside the routes
they replace; JSON lines appended to profiles/mla/bench_mla_append_ds.jsonl.  The protocol is benchmarks/bench_mla_sparse.py's: kernel
times come from a `rocprofv3 --kernel-trace --stats` child per shape (a fresh process, under its own `timeout -k 10`; the first
non-zero status ends the run), the sides ALTERNATE call by call in that child, a one-element kernel launched after every call marks
the call boundaries in the trace (it is not counted), the first 3 rounds are warm-up, and avg, min-max and stddev are reported per
call with the number of kernels a call launched.  Every side rotates over COPIES sets of sources and pools.

Shapes (bf16, H_kv = 1, paged at page 64, every sequence 1,024 keys long before the call, index keys at d_I = 128):
  decode_b128   128 sequences, one new token each (the fixed form);
  mixed_1024    one 1,024-token chunk beside 63 one-token decodes, packed (the _varlen form);
  prefill_8192  one 8,192-token chunk (the fixed form).
Sides:
  ds_hip     mla_kvcache_append[_varlen](kv_format="fp8_ds"): one launch, 1,152 bytes read and 656 written per token;
  ds_torch   the route it replaces: quantize_mla_cache_ds on the new rows, then an indexed copy of the 656-byte rows through the table
             (the flat row numbers prepared outside the timed calls);
  e4m3_hip   the one-descale e4m3 mla_kvcache_append[_varlen] on the same rows: 1,152 bytes read, 576 written, no reduction;
  idx_hip    mla_indexer_append[_varlen] into an e4m3 k_idx with k_scale;
  idx_torch  quantize_index_keys on the new rows, then indexed copies of bytes and scales.
No side rotates anything: the torch route has no rotary, so the HIP sides are called without tables."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "mla", "bench_mla_append_ds.jsonl")
PAGE, CONTEXT, D_I, COPIES, WARM = 64, 1024, 128, 4, 3
CASES = {"decode_b128": [1] * 128, "mixed_1024": [1024] + [1] * 63, "prefill_8192": [8192]}  # new tokens per sequence
SIDES = ("ds_hip", "ds_torch", "e4m3_hip", "idx_hip", "idx_torch")
MARK = "erfinv"  # the marker kernel: an operation no side launches


def run_child(name, iters):
    """The traced child: COPIES sets of tensors, then one call of every side in turn, a mark after each."""
    import torch
    import flash_attention_dlrs_amd as fa
    dev, bf = torch.device("cuda:0"), torch.bfloat16
    new = CASES[name]
    B, total, packed = len(new), sum(new), len(set(new)) > 1
    mb = (CONTEXT + max(new) + PAGE - 1) // PAGE
    nb = B * mb
    table = torch.randperm(nb, device=dev).to(torch.int32).view(B, mb)
    lens = torch.full((B,), CONTEXT, dtype=torch.int32, device=dev)
    cu = torch.tensor([0] + new, device=dev).cumsum(0).to(torch.int32)
    # the pool row of every new token, for the torch routes
    seq = torch.repeat_interleave(torch.arange(B, device=dev), torch.tensor(new, device=dev))
    pos = CONTEXT + torch.arange(total, device=dev) - cu[:-1].long()[seq]
    flat = table.long()[seq, pos // PAGE] * PAGE + pos % PAGE
    lead = (total, 1) if packed else (B, 1, new[0])
    sets = []
    for _ in range(COPIES):
        sets.append(dict(kv=torch.randn(*lead, 576, device=dev).to(bf), k=torch.randn(*(lead[:1] + lead[2:]), D_I, device=dev).to(bf),
                         ds=torch.zeros(nb, 1, PAGE, 656, dtype=torch.uint8, device=dev),
                         e4=torch.zeros(nb, 1, PAGE, 576, device=dev).to(torch.float8_e4m3fn),
                         k8=torch.zeros(nb, PAGE, D_I, device=dev).to(torch.float8_e4m3fn), ks=torch.zeros(nb, PAGE, device=dev)))
    one = torch.ones(B, 1, device=dev)
    mark = torch.zeros(1, device=dev)

    def run(side, s):
        if side == "ds_hip" or side == "e4m3_hip":
            cache, kw = (s["ds"], dict(kv_format="fp8_ds")) if side == "ds_hip" else (s["e4"], dict(kv_descale=one))
            if packed:
                fa.mla_kvcache_append_varlen(cache, s["kv"], cu, max(new), lens, block_table=table, **kw)
            else:
                fa.mla_kvcache_append(cache, s["kv"], lens, block_table=table, **kw)
        elif side == "ds_torch":
            s["ds"].view(-1, 656).index_copy_(0, flat, fa.quantize_mla_cache_ds(s["kv"]).view(-1, 656))
        elif side == "idx_hip":
            if packed:
                fa.mla_indexer_append_varlen(s["k8"], s["k"], cu, max(new), lens, k_scale=s["ks"], block_table=table)
            else:
                fa.mla_indexer_append(s["k8"], s["k"], lens, k_scale=s["ks"], block_table=table)
        else:
            k8, sc = fa.quantize_index_keys(s["k"], torch.float8_e4m3fn)
            s["k8"].view(torch.uint8).view(-1, D_I).index_copy_(0, flat, k8.view(torch.uint8).view(-1, D_I))
            s["ks"].view(-1).index_copy_(0, flat, sc.view(-1))

    torch.cuda.synchronize()
    mark.erfinv_()  # the first mark: what lies before it is set-up
    rounds = iters + WARM
    for r in range(rounds):
        for side in SIDES:
            run(side, sets[r % COPIES])
            mark.erfinv_()
    torch.cuda.synchronize()
    print(json.dumps(dict(case=name, rounds=rounds, B=B, total_new=total, packed=packed, page=PAGE, context=CONTEXT)))


def call_times(out, total):
    """(kernel microseconds, kernel count, kernel names) of each of the last `total` calls: the trace cut at the marks."""
    trace = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
    rows = sorted(csv.DictReader(open(trace[0])), key=lambda r: int(r["Start_Timestamp"]))
    marks = [k for k, r in enumerate(rows) if MARK in r["Kernel_Name"]][-(total + 1):]
    assert len(marks) == total + 1 and marks[-1] == len(rows) - 1, (len(marks), total, marks[-1], len(rows))
    calls = []
    for lo, hi in zip(marks, marks[1:]):
        seg = rows[lo + 1:hi]
        assert seg, "two marks with no kernel between them"
        calls.append((sum(int(x["End_Timestamp"]) - int(x["Start_Timestamp"]) for x in seg) / 1e3, len(seg), sorted({x["Kernel_Name"][:60] for x in seg})))
    return calls


def stats(calls):
    us = [t for t, _, _ in calls[WARM:]]
    avg = sum(us) / len(us)
    return dict(avg_us=round(avg, 2), min_us=round(min(us), 2), max_us=round(max(us), 2),
                stddev_us=round((sum((u - avg) ** 2 for u in us) / len(us)) ** 0.5, 2), calls=len(us), launches=max(n for _, n, _ in calls),
                kernels=sorted({k for _, _, ks in calls for k in ks}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rocprof", metavar="DIR", default=os.path.join(ROOT, "bench_out", "mla_append_ds_traces"))
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--child-case", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    if args.child_case:
        return run_child(args.child_case, args.iters)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fh:
        for name in args.cases.split(","):
            out = os.path.join(args.rocprof, name)
            os.makedirs(out, exist_ok=True)
            cmd = ["timeout", "-k", "10", str(args.child_timeout), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out,
                   "--", sys.executable, os.path.abspath(__file__), "--iters", str(args.iters), "--child-case", name]
            p = subprocess.run(cmd, capture_output=True, text=True)
            if p.returncode != 0:  # a failed child ends the run: nothing more is started on the GPU
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
                sys.exit(p.returncode)
            info = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
            calls = call_times(out, info["rounds"] * len(SIDES))
            sides = {side: stats(calls[k::len(SIDES)]) for k, side in enumerate(SIDES)}
            line = json.dumps(dict(kind="append_ds", **{k: v for k, v in info.items() if k != "rounds"},
                                   ds_hip_over_torch=round(sides["ds_hip"]["avg_us"] / sides["ds_torch"]["avg_us"], 4),
                                   ds_hip_over_e4m3=round(sides["ds_hip"]["avg_us"] / sides["e4m3_hip"]["avg_us"], 4),
                                   e4m3_ranges_overlap=sides["ds_hip"]["max_us"] >= sides["e4m3_hip"]["min_us"] and sides["e4m3_hip"]["max_us"] >= sides["ds_hip"]["min_us"],
                                   idx_hip_over_torch=round(sides["idx_hip"]["avg_us"] / sides["idx_torch"]["avg_us"], 4), **sides))
            print(line, flush=True)
            fh.write(line + "\n")
            fh.flush()


if __name__ == "__main__":
    main()
