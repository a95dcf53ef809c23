#!/usr/bin/env python3
"""Local (sliding-window) attention timing: forward and backward of fa2_fwd_window / fa2_bwd_window against the FULL causal
problem on the default kernels (fa2_fwd / fa2_bwd, causal) on the same device, in interleaved rounds (HIP events).

TFLOP/s count the VISIBLE (query, key) pairs: 4 B H d pairs for the forward, 2.5 x that for the backward (the project's
convention, benchmarks/bench_bwd.py).  One JSON line per shape and direction."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flash_attention_dlrs_amd import flash_attention_backward, flash_attention_forward  # noqa: E402
from flash_attention_dlrs_amd.flash_attention_torch import normalize_window  # noqa: E402


def visible_pairs(N, causal, window):
    """number of (query, key) pairs with key j visible to query i (include/fa2_fwd.h)"""
    causal, w = normalize_window(N, causal, window)
    if w is None:
        return N * (N + 1) // 2 if causal else N * N
    left, right = w
    total = 0
    for i in range(N):
        total += min(N - 1, i + right) - max(0, i - left) + 1
    return total


def time_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def interleaved(fns, iters, rounds):
    """median ms of each callable over `rounds` interleaved rounds (after a warm-up of each)"""
    for f in fns:
        f()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(rounds):
        for k, f in enumerate(fns):
            ts[k].append(time_ms(f, iters))
    return [sorted(t)[len(t) // 2] for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4)
    ap.add_argument("--H", type=int, default=32)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--Ns", default="4096,16384")
    ap.add_argument("--windows", default="256:0,1024:0,4096:0,512:512", help="left:right pairs; right = 0 runs causal")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, H, d = args.B, args.H, args.d
    scale = d ** -0.5
    for N in (int(n) for n in args.Ns.split(",")):
        torch.manual_seed(0)
        Q, K, V, dO = ((torch.randn(B, H, N, d, device=dev) * 0.8).to(torch.bfloat16) for _ in range(4))
        Oc, Lc = flash_attention_forward(Q, K, V, dev, causal=True, scale=scale)
        full = visible_pairs(N, True, None)
        for spec in args.windows.split(","):
            left, right = (int(x) for x in spec.split(":"))
            causal = right == 0
            window = (left, right)
            Ow, Lw = flash_attention_forward(Q, K, V, dev, causal=causal, scale=scale, window=window)
            pairs = visible_pairs(N, causal, window)
            fwd_w, fwd_c = interleaved([
                lambda: flash_attention_forward(Q, K, V, dev, causal=causal, scale=scale, window=window),
                lambda: flash_attention_forward(Q, K, V, dev, causal=True, scale=scale)], args.iters, args.rounds)
            bwd_w, bwd_c = interleaved([
                lambda: flash_attention_backward(Q, K, V, Ow, dO, Lw, dev, causal=causal, scale=scale, window=window),
                lambda: flash_attention_backward(Q, K, V, Oc, dO, Lc, dev, causal=True, scale=scale)], args.iters, args.rounds)
            fl = 4.0 * B * H * d * pairs
            for direction, tw, tc, f, fc in (("fwd", fwd_w, fwd_c, fl, 4.0 * B * H * d * full),
                                             ("bwd", bwd_w, bwd_c, 2.5 * fl, 10.0 * B * H * d * full)):
                print(json.dumps({"shape": f"bf16 B{B} H{H} N{N} d{d}", "window": list(window), "causal": causal,
                                  "direction": direction, "visible_pairs": pairs, "pairs_vs_causal": round(pairs / full, 4),
                                  "ms": round(tw, 4), "tflops": round(f / tw / 1e9, 1),
                                  "full_causal_ms": round(tc, 4), "full_causal_tflops": round(fc / tc / 1e9, 1),
                                  "ratio_vs_full_causal": round(tw / tc, 3)}), flush=True)


if __name__ == "__main__":
    main()
