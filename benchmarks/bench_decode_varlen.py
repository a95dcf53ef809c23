#!/usr/bin/env python3
"""Kernel times of variable-length queries over the KV cache (flash_attention_varlen_kvcache_forward) against the two routes it
replaces, with the protocol of benchmarks/bench_decode.py: one `rocprofv3 --kernel-trace --stats` child per shape (the program
after `--`), the sides alternating call by call, K / V rotating over more copies than the 256 MiB last-level cache holds, 3 warm
calls per side, per-call kernel times read off the kernel trace.

Sides:
  new     the packed call;
  padded  flash_attention_kvcache_forward with every sequence padded to the longest chunk (Q rows past n_q(b) repeat the last
          row; the cache lengths are the same, so the padded rows attend as later positions would) -- the VALU form once
          g * N_q > 64;
  gather  the cache gathered into a packed (total_k, H_kv, d) K / V with one index_select each, then
          flash_attention_varlen_forward; the gather kernels are counted.  Not available over an fp8 cache.

bf16, d 128, causal.  Results: profiles/decode/bench_varlen_q.jsonl.

  python benchmarks/bench_decode_varlen.py --rocprof /tmp/varlen_q [--cases a_chunk512,...] [--iters 10]
"""
import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "decode", "bench_varlen_q.jsonl")
LLC_BYTES = 256 << 20

# name: (H, H_kv, [(n_q, N_k)] per sequence, page_size or 0, fp8 cache)
CASES = {
    "a_chunk512": (32, 8, [(512, 4096)] * 4, 0, False),
    "b_chunk2048": (32, 8, [(2048, 32768)], 0, False),
    "c_mixed": (32, 8, [(1024, 8192)] + [(1, 4096)] * 63, 0, False),
    "d_spec8": (32, 2, [(8, 4096)] * 16, 0, False),
    "e_chunk512_paged256": (32, 8, [(512, 4096)] * 4, 256, False),
    "e_chunk512_e4m3": (32, 8, [(512, 4096)] * 4, 0, True),
}
D = 128


def build(name, torch):
    """-> (sides {name: callable}, info)"""
    import flash_attention_dlrs_amd as fa
    dev = torch.device("cuda:0")
    H, H_kv, seqs, page, fp8 = CASES[name]
    B = len(seqs)
    n_q, n_k = [s[0] for s in seqs], [s[1] for s in seqs]
    cap, max_q, total_q = max(n_k), max(n_q), sum(n_q)
    g = torch.Generator(device="cpu").manual_seed(1)
    Q = (torch.randn(total_q, H, D, generator=g) * 0.5).to(torch.bfloat16).to(dev)
    cu_q = torch.tensor([0] + torch.tensor(n_q).cumsum(0).tolist(), dtype=torch.int32, device=dev)
    cu_k = torch.tensor([0] + torch.tensor(n_k).cumsum(0).tolist(), dtype=torch.int32, device=dev)
    lens = torch.tensor(n_k, dtype=torch.int32, device=dev)
    # padded Q (B, H, max_q, d): rows past n_q(b) repeat the sequence's last row
    Qp = torch.empty(B, max_q, H, D, dtype=torch.bfloat16, device=dev)
    for b in range(B):
        rows = Q[int(cu_q[b]):int(cu_q[b + 1])]
        Qp[b, :n_q[b]] = rows
        Qp[b, n_q[b]:] = rows[-1:]
    Qp = Qp.transpose(1, 2)
    live_bytes = 2 * sum(n_k) * H_kv * D * (1 if fp8 else 2)
    copies = max(2, -(-2 * LLC_BYTES // live_bytes) + 1)
    caches = []
    for c in range(copies):  # flash-attn layouts: (B, S, H_kv, d), or a pool (num_blocks, page, H_kv, d) behind a permuted table
        K = torch.empty(B, cap, H_kv, D, dtype=torch.bfloat16, device=dev).normal_(0, 0.5)
        V = torch.empty(B, cap, H_kv, D, dtype=torch.bfloat16, device=dev).normal_(0, 0.5)
        kw = {}
        if page:
            mb = cap // page
            perm = torch.randperm(B * mb, generator=torch.Generator().manual_seed(c)).to(dev)
            table = perm.view(B, mb).to(torch.int32).contiguous()
            Kp, Vp = torch.empty(B * mb, page, H_kv, D, dtype=K.dtype, device=dev), torch.empty(B * mb, page, H_kv, D, dtype=K.dtype, device=dev)
            Kp[perm] = K.view(B * mb, page, H_kv, D)
            Vp[perm] = V.view(B * mb, page, H_kv, D)
            K, V, kw = Kp, Vp, dict(block_table=table)
            j = torch.cat([torch.arange(n, device=dev) for n in n_k])
            b = torch.cat([torch.full((n,), i, device=dev) for i, n in enumerate(n_k)])
            index = table.long()[b, j // page] * page + j % page
        else:
            index = torch.cat([torch.arange(n, device=dev) + i * cap for i, n in enumerate(n_k)])
        if fp8:
            K, dk = fa.quantize_kv_cache(K.transpose(1, 2), torch.float8_e4m3fn)
            V, dv = fa.quantize_kv_cache(V.transpose(1, 2), torch.float8_e4m3fn)
            kw.update(k_descale=dk, v_descale=dv)
            caches.append((K, V, kw, None))
        else:
            caches.append((K.transpose(1, 2), V.transpose(1, 2), kw, (K.view(-1, H_kv, D), V.view(-1, H_kv, D), index)))
    scale = D ** -0.5
    turn = {"new": 0, "padded": 0, "gather": 0}

    def pick(side):
        turn[side] += 1
        return caches[turn[side] % copies]

    def new():
        K, V, kw, _ = pick("new")
        return fa.flash_attention_varlen_kvcache_forward(Q, K, V, cu_q, max_q, lens, dev, causal=True, scale=scale, **kw)

    def padded():
        K, V, kw, _ = pick("padded")
        return fa.flash_attention_kvcache_forward(Qp, K, V, lens, dev, causal=True, scale=scale, **kw)

    def gather():
        Kf, Vf, index = pick("gather")[3]
        return fa.flash_attention_varlen_forward(Q, Kf.index_select(0, index), Vf.index_select(0, index), cu_q, cu_k, max_q, cap, dev,
                                                 causal=True, scale=scale)

    sides = {"new": new, "padded": padded}
    if not fp8:
        sides["gather"] = gather
    info = dict(case=name, B=B, H=H, H_kv=H_kv, d=D, total_q=total_q, max_seqlen_q=max_q, capacity=cap, page_size=page,
                kv_dtype="e4m3" if fp8 else "bf16", copies=copies, live_kv_bytes=live_bytes)
    return sides, info


def run_pass(name, iters):
    """the traced child: the sides alternate call by call; the order of a round is what the parent reads the trace by"""
    import torch
    sides, info = build(name, torch)
    torch.cuda.synchronize()
    for _ in range(iters + 3):
        for f in sides.values():
            f()
            torch.cuda.synchronize()
    print(json.dumps(dict(calls=iters + 3, sides=list(sides), **info)))


VQ_KERNEL = re.compile(r"Lb[01]ELb1E|<[^>]*\b(?:true|false), true\b")  # mangled or demangled: PAGED, then VQ = true


def side_times(out, info):
    """per-call kernel time of every side.  The calls are cut out of the trace in dispatch order -- a decode split kernel opens a
    call, the combine joins it, the first other kernel behind a decode call opens a gather call -- and belong to the sides in the
    order the child ran them; then the kernels of each side are checked by name: `new` ran the query-tiled matrix kernel (every shape here is one of
    its shapes) and `padded` the VALU kernel of the fixed call, `gather` no decode kernel at all."""
    trace = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
    rows = sorted(csv.DictReader(open(trace[0])), key=lambda r: int(r["Start_Timestamp"]))
    # the calls in dispatch order: a new call starts at every split kernel of a decode side and at the first kernel of a gather
    calls, cur = [], None
    for r in rows:
        k = r["Kernel_Name"]
        split = "fa2_decode" in k and "combine" not in k and "append" not in k
        if split or cur is None or (cur["decode"] and "fa2_decode" not in k):
            cur = dict(decode=split, kernels=[])
            calls.append(cur)
        cur["kernels"].append(r)
    order, n = info["sides"], info["calls"]
    calls = calls[-len(order) * n:]  # (whatever ran while the inputs were built comes first)
    assert len(calls) == len(order) * n, (len(calls), len(order), n)
    res = {}
    for s, side in enumerate(order):
        mine = calls[s::len(order)]
        assert all(c["decode"] == (side != "gather") for c in mine), side
        splits = {c["kernels"][0]["Kernel_Name"] for c in mine} if side != "gather" else set()
        if side == "new":  # fa2_decode_mfma16_kernel<T, C, PAGED, VQ = true, ...>: "Lb1E" is the second bool of the mangled name
            assert all("fa2_decode_mfma16_kernel" in k and VQ_KERNEL.search(k) for k in splits), splits
        if side == "padded":
            assert all("fa2_decode_generic_kernel" in k for k in splits), splits
        us = [sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in c["kernels"]) / 1e3 for c in mine[3:]]
        avg = sum(us) / len(us)
        res[side] = dict(avg_us=round(avg, 2), min_us=round(min(us), 2), max_us=round(max(us), 2),
                         stddev_us=round((sum((u - avg) ** 2 for u in us) / len(us)) ** 0.5, 2),
                         kernels=sorted({r["Kernel_Name"][:80] for c in mine for r in c["kernels"]}))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rocprof", metavar="DIR", help="where the traces go (required unless --pass-case)")
    ap.add_argument("--child-timeout", type=int, default=300)
    ap.add_argument("--pass-case", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    if args.pass_case:
        return run_pass(args.pass_case, args.iters)
    if not args.rocprof:
        ap.error("--rocprof DIR is required")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fh:
        for name in args.cases.split(","):
            out = os.path.join(args.rocprof, name)
            os.makedirs(out, exist_ok=True)
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable,
                   os.path.abspath(__file__), "--iters", str(args.iters), "--pass-case", name]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.child_timeout)
            if p.returncode != 0:  # a failed child ends the run: nothing more is started on the GPU
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
                sys.exit(p.returncode)
            info = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
            sides = side_times(out, info)
            rec = dict(kind="kernels_varlen_q", **info, **sides)
            rec["padded_over_new"] = round(sides["padded"]["avg_us"] / sides["new"]["avg_us"], 3)
            if "gather" in sides:
                rec["gather_over_new"] = round(sides["gather"]["avg_us"] / sides["new"]["avg_us"], 3)
            line = json.dumps(rec)
            print(line, flush=True)
            fh.write(line + "\n")
            fh.flush()


if __name__ == "__main__":
    main()
