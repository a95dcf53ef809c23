#!/usr/bin/env python3
"""Variable-length (packed) attention timing, bf16 H32 d128, HIP events in interleaved rounds; one JSON line per case and
direction (results kept under profiles/varlen/).

  equal:  B sequences of N, varlen against the dense call with the same forced forward variant (the overhead of the offsets);
          the backward against the dense AUTO backward.
  skewed: a seeded log-uniform mix of lengths in [128, 8192] summing to ~64 Ki tokens, causal and not; varlen against
          (a) the dense AUTO call padded to B x max_len (timed only: its numbers are not the varlen ones) and
          (b) a loop of per-sequence dense AUTO calls.

TFLOP/s count the visible (query, key) pairs: 4 H d per pair forward, 2.5 x that backward (benchmarks/bench_bwd.py)."""
import argparse
import json
import math
import os
import random
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flash_attention_dlrs_amd import (flash_attention_backward, flash_attention_forward,  # noqa: E402
                                      flash_attention_varlen_backward, flash_attention_varlen_forward)


def time_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def interleaved(fns, iters, rounds):
    for f in fns:
        f()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(rounds):
        for k, f in enumerate(fns):
            ts[k].append(time_ms(f, iters))
    return [sorted(t)[len(t) // 2] for t in ts]


def pairs(lengths, causal):
    return sum(n * (n + 1) // 2 if causal else n * n for n in lengths)


def skewed_lengths(seed, total, lo=128, hi=8192):
    rng = random.Random(seed)
    out = []
    while sum(out) < total:
        n = int(math.exp(rng.uniform(math.log(lo), math.log(hi))))
        out.append(min(n, total - sum(out)) if total - sum(out) >= lo else lo)
    return out


def emit(**kw):
    print(json.dumps(kw), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--H", type=int, default=32)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--equal", default="8x2048,2x8192", help="BxN cases of the equal-length comparison")
    ap.add_argument("--total", type=int, default=65536)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--bwd-iters", type=int, default=1)
    ap.add_argument("--no-bwd", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    H, d = args.H, args.d
    scale = d ** -0.5
    mk = lambda *s: (torch.randn(*s, device=dev) * 0.8).to(torch.bfloat16)

    for spec in args.equal.split(","):
        B, N = (int(x) for x in spec.split("x"))
        torch.manual_seed(0)
        Qd, Kd, Vd, dOd = (mk(B, H, N, d) for _ in range(4))
        pack = lambda t: t.transpose(1, 2).reshape(B * N, H, d).contiguous()
        Q, K, V, dO = (pack(t) for t in (Qd, Kd, Vd, dOd))
        cu = torch.arange(0, B * N + 1, N, dtype=torch.int32, device=dev)
        for causal in (False, True):
            fl = 4.0 * H * d * pairs([N] * B, causal)
            for variant in ("mfma16d", "mfma16d_w4"):
                tv, td = interleaved([
                    lambda: flash_attention_varlen_forward(Q, K, V, cu, cu, N, N, dev, causal=causal, scale=scale, variant=variant),
                    lambda: flash_attention_forward(Qd, Kd, Vd, dev, causal=causal, scale=scale, variant=variant)],
                    args.iters, args.rounds)
                emit(case="equal", shape=f"bf16 B{B} H{H} N{N} d{d}", causal=causal, direction="fwd", variant=variant,
                     varlen_ms=round(tv, 4), dense_ms=round(td, 4), varlen_tflops=round(fl / tv / 1e9, 1),
                     ratio_varlen_vs_dense=round(tv / td, 3))
            if not args.no_bwd:
                O, L = flash_attention_varlen_forward(Q, K, V, cu, cu, N, N, dev, causal=causal, scale=scale)
                Od, Ld = flash_attention_forward(Qd, Kd, Vd, dev, causal=causal, scale=scale)
                tv, td = interleaved([
                    lambda: flash_attention_varlen_backward(Q, K, V, O, dO, L, cu, cu, N, N, dev, causal=causal, scale=scale),
                    lambda: flash_attention_backward(Qd, Kd, Vd, Od, dOd, Ld, dev, causal=causal, scale=scale)],
                    args.bwd_iters, args.rounds)
                emit(case="equal", shape=f"bf16 B{B} H{H} N{N} d{d}", causal=causal, direction="bwd", variant="auto",
                     varlen_ms=round(tv, 4), dense_ms=round(td, 4), varlen_tflops=round(2.5 * fl / tv / 1e9, 1),
                     ratio_varlen_vs_dense=round(tv / td, 3))

    lengths = skewed_lengths(args.seed, args.total)
    B, total, maxlen = len(lengths), sum(lengths), max(lengths)
    torch.manual_seed(1)
    Q, K, V, dO = (mk(total, H, d) for _ in range(4))
    cu = torch.tensor([0] + torch.tensor(lengths).cumsum(0).tolist(), dtype=torch.int32, device=dev)
    Qp, Kp, Vp, dOp = (mk(B, H, maxlen, d) for _ in range(4))  # the padded dense problem (timing only)
    starts = cu.tolist()
    seqs = [tuple(t[starts[b]:starts[b + 1]].transpose(0, 1).unsqueeze(0) for t in (Q, K, V, dO)) for b in range(B)]
    for causal in (False, True):
        real = pairs(lengths, causal)
        padded = pairs([maxlen] * B, causal)
        fl = 4.0 * H * d * real

        def loop_fwd():
            for q, k, v, _ in seqs:
                flash_attention_forward(q, k, v, dev, causal=causal, scale=scale)

        tv, tp, tl = interleaved([
            lambda: flash_attention_varlen_forward(Q, K, V, cu, cu, maxlen, maxlen, dev, causal=causal, scale=scale),
            lambda: flash_attention_forward(Qp, Kp, Vp, dev, causal=causal, scale=scale),
            loop_fwd], args.iters, args.rounds)
        common = dict(case="skewed", shape=f"bf16 H{H} d{d} total{total} B{B} max{maxlen}", seed=args.seed, causal=causal,
                      real_pairs=real, padded_pairs=padded, padded_vs_real=round(padded / real, 3))
        emit(**common, direction="fwd", varlen_ms=round(tv, 4), padded_dense_ms=round(tp, 4), per_seq_loop_ms=round(tl, 4),
             varlen_tflops=round(fl / tv / 1e9, 1), speedup_vs_padded=round(tp / tv, 3), speedup_vs_loop=round(tl / tv, 3))
        if args.no_bwd:
            continue
        O, L = flash_attention_varlen_forward(Q, K, V, cu, cu, maxlen, maxlen, dev, causal=causal, scale=scale)
        Op, Lp = flash_attention_forward(Qp, Kp, Vp, dev, causal=causal, scale=scale)
        fw = [flash_attention_forward(q, k, v, dev, causal=causal, scale=scale) for q, k, v, _ in seqs]

        def loop_bwd():
            for (q, k, v, g), (o, l) in zip(seqs, fw):
                flash_attention_backward(q, k, v, o, g, l, dev, causal=causal, scale=scale)

        tv, tp, tl = interleaved([
            lambda: flash_attention_varlen_backward(Q, K, V, O, dO, L, cu, cu, maxlen, maxlen, dev, causal=causal, scale=scale),
            lambda: flash_attention_backward(Qp, Kp, Vp, Op, dOp, Lp, dev, causal=causal, scale=scale),
            loop_bwd], args.bwd_iters, args.rounds)
        emit(**common, direction="bwd", varlen_ms=round(tv, 4), padded_dense_ms=round(tp, 4), per_seq_loop_ms=round(tl, 4),
             varlen_tflops=round(2.5 * fl / tv / 1e9, 1), speedup_vs_padded=round(tp / tv, 3), speedup_vs_loop=round(tl / tv, 3))


if __name__ == "__main__":
    main()
