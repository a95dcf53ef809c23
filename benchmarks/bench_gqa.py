#!/usr/bin/env python3
"""Grouped-query attention timing, bf16, HIP events in interleaved rounds; one JSON line per case, direction and causal flag
(results kept under profiles/gqa/).

Each case compares
  (a) gqa:        the GQA call on K, V with H_kv heads;
  (b) mha:        the MHA call at the same H on K, V expanded beforehand (the expansion not timed);
  (c) workaround: repeat_interleave of K and V, the MHA call and (backward) the group sum of dK / dV, all timed.
Cases: B4 H32 H_kv8 N4096, B2 H64 H_kv8 N8192, B4 H32 H_kv1 N4096 (MQA), one d = 64 case, one non-mergeable (B, N, H, d)
view, and a skewed varlen mix with H_kv 8.  TFLOP/s count the visible (query, key) pairs: 4 H d per pair forward, 2.5 x that
backward (benchmarks/bench_bwd.py)."""
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
from flash_attention_dlrs_amd.flash_attention_torch import group_sum  # noqa: E402


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


def emit(**kw):
    print(json.dumps(kw), flush=True)


def skewed_lengths(seed, total, lo=128, hi=8192):
    rng = random.Random(seed)
    out = []
    while sum(out) < total:
        n = int(math.exp(rng.uniform(math.log(lo), math.log(hi))))
        out.append(min(n, total - sum(out)) if total - sum(out) >= lo else lo)
    return out


def dense_case(name, B, H, H_kv, N, d, layout, args, dev):
    g = H // H_kv
    scale = d ** -0.5
    mk = lambda h: (torch.randn(B, N, h, d, device=dev) * 0.8).to(torch.bfloat16)  # noqa: E731
    if layout == "bnhd":  # a (B, N, H, d) tensor viewed as (B, H, N, d): not mergeable for B > 1
        Q, K, V, dO = (mk(h).transpose(1, 2) for h in (H, H_kv, H_kv, H))
    else:
        Q, K, V, dO = (mk(h).transpose(1, 2).contiguous() for h in (H, H_kv, H_kv, H))
    Kx, Vx = (t.repeat_interleave(g, dim=1) for t in (K, V))
    for causal in (False, True):
        flops = 4 * B * H * d * (N * (N + 1) // 2 if causal else N * N)
        fa = lambda: flash_attention_forward(Q, K, V, dev, causal=causal, scale=scale)  # noqa: E731
        fb = lambda: flash_attention_forward(Q, Kx, Vx, dev, causal=causal, scale=scale)  # noqa: E731

        def fc():
            ke, ve = K.repeat_interleave(g, dim=1), V.repeat_interleave(g, dim=1)
            return flash_attention_forward(Q, ke, ve, dev, causal=causal, scale=scale)
        ta, tb, tc = interleaved([fa, fb, fc], args.iters, args.rounds)
        emit(case=name, dir="fwd", B=B, H=H, H_kv=H_kv, N=N, d=d, layout=layout, causal=causal, gqa_ms=round(ta, 4),
             mha_ms=round(tb, 4), workaround_ms=round(tc, 4), gqa_tflops=round(flops / ta / 1e9, 1),
             gqa_over_mha=round(ta / tb, 3), gqa_over_workaround=round(ta / tc, 3))
        if args.no_bwd:
            continue
        O, L = fa()
        Om, Lm = fb()
        ba = lambda: flash_attention_backward(Q, K, V, O, dO, L, dev, causal=causal, scale=scale)  # noqa: E731
        bb = lambda: flash_attention_backward(Q, Kx, Vx, Om, dO, Lm, dev, causal=causal, scale=scale)  # noqa: E731

        def bc():
            ke, ve = K.repeat_interleave(g, dim=1), V.repeat_interleave(g, dim=1)
            dq, dk, dv = flash_attention_backward(Q, ke, ve, Om, dO, Lm, dev, causal=causal, scale=scale)
            return dq, group_sum(dk, H_kv), group_sum(dv, H_kv)
        ta, tb, tc = interleaved([ba, bb, bc], args.bwd_iters, args.rounds)
        emit(case=name, dir="bwd", B=B, H=H, H_kv=H_kv, N=N, d=d, layout=layout, causal=causal, gqa_ms=round(ta, 4),
             mha_ms=round(tb, 4), workaround_ms=round(tc, 4), gqa_tflops=round(2.5 * flops / ta / 1e9, 1),
             gqa_over_mha=round(ta / tb, 3), gqa_over_workaround=round(ta / tc, 3),
             dkdv_workgroups=B * H_kv * ((N + 127) // 128))
        del O, L, Om, Lm
    del Q, K, V, dO, Kx, Vx
    torch.cuda.empty_cache()


def varlen_case(args, dev, H=32, H_kv=8, d=128):
    g = H // H_kv
    lengths = skewed_lengths(args.seed, args.total)
    cu = torch.tensor([0] + list(torch.tensor(lengths).cumsum(0).tolist()), dtype=torch.int32, device=dev)
    T, mx = sum(lengths), max(lengths)
    scale = d ** -0.5
    Q, dO = ((torch.randn(T, H, d, device=dev) * 0.8).to(torch.bfloat16) for _ in range(2))
    K, V = ((torch.randn(T, H_kv, d, device=dev) * 0.8).to(torch.bfloat16) for _ in range(2))
    Kx, Vx = (t.repeat_interleave(g, dim=1) for t in (K, V))
    for causal in (False, True):
        flops = 4 * H * d * sum(n * (n + 1) // 2 if causal else n * n for n in lengths)
        fwd = lambda k, v: flash_attention_varlen_forward(Q, k, v, cu, cu, mx, mx, dev, causal=causal, scale=scale)  # noqa: E731

        def fc():
            return fwd(K.repeat_interleave(g, dim=1), V.repeat_interleave(g, dim=1))
        ta, tb, tc = interleaved([lambda: fwd(K, V), lambda: fwd(Kx, Vx), fc], args.iters, args.rounds)
        common = dict(case="varlen_skewed", B=len(lengths), H=H, H_kv=H_kv, total=T, max_len=mx, d=d, causal=causal)
        emit(dir="fwd", **common, gqa_ms=round(ta, 4), mha_ms=round(tb, 4), workaround_ms=round(tc, 4),
             gqa_tflops=round(flops / ta / 1e9, 1), gqa_over_mha=round(ta / tb, 3), gqa_over_workaround=round(ta / tc, 3))
        if args.no_bwd:
            continue
        O, L = fwd(K, V)
        bwd = lambda k, v: flash_attention_varlen_backward(Q, k, v, O, dO, L, cu, cu, mx, mx, dev, causal=causal,  # noqa: E731
                                                           scale=scale)

        def bc():
            dq, dk, dv = bwd(K.repeat_interleave(g, dim=1), V.repeat_interleave(g, dim=1))
            return dq, dk.unflatten(1, (H_kv, g)).sum(2), dv.unflatten(1, (H_kv, g)).sum(2)
        ta, tb, tc = interleaved([lambda: bwd(K, V), lambda: bwd(Kx, Vx), bc], args.bwd_iters, args.rounds)
        emit(dir="bwd", **common, gqa_ms=round(ta, 4), mha_ms=round(tb, 4), workaround_ms=round(tc, 4),
             gqa_tflops=round(2.5 * flops / ta / 1e9, 1), gqa_over_mha=round(ta / tb, 3), gqa_over_workaround=round(ta / tc, 3))


CASES = {  # name: (B, H, H_kv, N, d, layout)
    "b4h32kv8n4096": (4, 32, 8, 4096, 128, "contig"),
    "b2h64kv8n8192": (2, 64, 8, 8192, 128, "contig"),
    "mqa_b4h32kv1n4096": (4, 32, 1, 4096, 128, "contig"),
    "d64_b4h32kv8n4096": (4, 32, 8, 4096, 64, "contig"),
    "bnhd_b4h32kv8n4096": (4, 32, 8, 4096, 128, "bnhd"),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(list(CASES) + ["varlen"]))
    ap.add_argument("--total", type=int, default=65536)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--bwd-iters", type=int, default=2)
    ap.add_argument("--no-bwd", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    for name in args.cases.split(","):
        if name == "varlen":
            varlen_case(args, dev)
        else:
            dense_case(name, *CASES[name], args, dev)


if __name__ == "__main__":
    main()
