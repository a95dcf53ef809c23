#!/usr/bin/env python3
"""Timing of the indexer's front end (mla_indexer_prepare_queries and the rotary / hadamard keywords of mla_indexer_append,
fa2_indexer_prep.hip) beside the torch route an engine runs today; JSON lines appended to profiles/mla/bench_mla_indexer_prepare.jsonl.
The protocol is benchmarks/bench_mla_indexer.py's and bench_mla_append_ds.py's: kernel times come from a `rocprofv3 --kernel-trace
--stats` child per shape (a fresh process, under its own `timeout -k 10`; the first non-zero status ends the run), the sides ALTERNATE
call by call in that child, a one-element kernel launched after every call marks the call boundaries in the trace (it is not counted),
the first 3 rounds are warm-up, and avg, min-max and stddev are reported per call with the number of kernels a call launched.  Every
side rotates over COPIES sets of sources and caches.

Shapes (bf16, H_I = 64, d_I = 128, rotary_dim 64 in the half pairing, e4m3 outputs, a contiguous key cache, every sequence 1,024 keys
long before the step):
  decode_b1, decode_b16, decode_b128   one new token a sequence;
  chunk_1024                           one sequence, a 1,024-token chunk.
Sides:
  q_hip     mla_indexer_prepare_queries: one launch, 256 bytes read and 128 + 4 written a row;
  q_torch   apply_rotary, a matmul with H_128 / sqrt(128) in bf16, quantize_index_keys, the multiply into the weights;
  k_hip     mla_indexer_append(rotary_cos, rotary_sin, hadamard=True): one launch, lengths included;
  k_torch   apply_rotary, the matmul, then mla_indexer_append, which quantises (one launch of the quantising append)."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "mla", "bench_mla_indexer_prepare.jsonl")
CONTEXT, H_I, D_I, RD, COPIES, WARM = 1024, 64, 128, 64, 4, 3
CASES = {"decode_b1": (1, 1), "decode_b16": (16, 1), "decode_b128": (128, 1), "chunk_1024": (1, 1024)}  # (B, new tokens a sequence)
SIDES = ("q_hip", "q_torch", "k_hip", "k_torch")
MARK = "erfinv"  # the marker kernel: an operation no side launches


def run_child(name, iters):
    """The traced child: COPIES sets of tensors, then one call of every side in turn, a mark after each."""
    import torch
    import flash_attention_dlrs_amd as fa
    dev, bf, e4 = torch.device("cuda:0"), torch.bfloat16, torch.float8_e4m3fn
    B, N = CASES[name]
    S_k = CONTEXT + N
    before = torch.full((B,), CONTEXT, dtype=torch.int32, device=dev)
    after = before + N
    ang = torch.rand(S_k, RD // 2, device=dev) * 6.28
    cos, sin = ang.cos().to(bf), ang.sin().to(bf)
    had = torch.ones(1, 1, device=dev)
    for _ in range(7):
        had = torch.kron(torch.tensor([[1.0, 1.0], [1.0, -1.0]], device=dev), had)
    had = (had * D_I ** -0.5).to(bf)
    pos = CONTEXT + torch.arange(N, device=dev)
    sets = []
    for _ in range(COPIES):
        sets.append(dict(q=torch.randn(B, H_I, N, D_I, device=dev).to(bf), w=torch.rand(B, H_I, N, device=dev),
                         k=torch.randn(B, N, D_I, device=dev).to(bf), k8=torch.zeros(B, S_k, D_I, device=dev).to(e4),
                         ks=torch.zeros(B, S_k, device=dev)))
    mark = torch.zeros(1, device=dev)

    def run(side, s):
        if side == "q_hip":
            fa.mla_indexer_prepare_queries(s["q"], s["w"], after, weight_scale=0.125, rotary_cos=cos, rotary_sin=sin)
        elif side == "q_torch":
            q8, scale = fa.quantize_index_keys(fa.apply_rotary(s["q"], cos, sin, pos) @ had, e4)
            (s["w"] * 0.125) * scale
        elif side == "k_hip":
            fa.mla_indexer_append(s["k8"], s["k"], before, k_scale=s["ks"], rotary_cos=cos, rotary_sin=sin, hadamard=True)
        else:
            fa.mla_indexer_append(s["k8"], fa.apply_rotary(s["k"], cos, sin, pos) @ had, before, k_scale=s["ks"])

    torch.cuda.synchronize()
    mark.erfinv_()  # the first mark: what lies before it is set-up
    rounds = iters + WARM
    for r in range(rounds):
        for side in SIDES:
            run(side, sets[r % COPIES])
            mark.erfinv_()
    torch.cuda.synchronize()
    print(json.dumps(dict(case=name, rounds=rounds, B=B, N_new=N, H_I=H_I, context=CONTEXT)))


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
    ap.add_argument("--rocprof", metavar="DIR", default=os.path.join(ROOT, "bench_out", "mla_indexer_prepare_traces"))
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
            overlap = lambda a, b: sides[a]["max_us"] >= sides[b]["min_us"] and sides[b]["max_us"] >= sides[a]["min_us"]
            line = json.dumps(dict(kind="indexer_prepare", **{k: v for k, v in info.items() if k != "rounds"},
                                   q_hip_over_torch=round(sides["q_hip"]["avg_us"] / sides["q_torch"]["avg_us"], 4),
                                   k_hip_over_torch=round(sides["k_hip"]["avg_us"] / sides["k_torch"]["avg_us"], 4),
                                   q_ranges_overlap=overlap("q_hip", "q_torch"), k_ranges_overlap=overlap("k_hip", "k_torch"), **sides))
            print(line, flush=True)
            fh.write(line + "\n")
            fh.flush()


if __name__ == "__main__":
    main()
