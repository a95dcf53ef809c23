#!/usr/bin/env python3
"""The packed (ragged) KV-cache append (fa2_kvcache_append_varlen) against the route it replaces, by device events in the style of
bench_decode.py --append; bf16, d 128, H_kv 8, rotary on.  JSON lines appended to profiles/decode/bench_append_varlen.jsonl.

    python benchmarks/bench_append_varlen.py [--shapes a,b,c,d,e] [--iters 50] [--rounds 5] [--graph]

Shapes: (a) 4 chunks of 512 tokens into caches holding 4096 keys; (b) one chunk of 1024 beside 63 one-token decodes; (c) 64
one-token decodes, a uniform batch; (d) shape (a) behind 256-key pages; (e) shape (a) into an e4m3 cache.

Sides, alternated in one process, every call on preallocated outputs through the ctypes launchers (no Python argument checks in
the timed loop): `packed`, the new call; `grouped`, one fa2_kvcache_append per group of sequences that bring the same number of
tokens, on batch-axis views of the cache (table rows when paged), of the lengths and of the descales; on (c) also `fixed`, the
existing call at N_new = 1 on the whole tensors.  cache_seqlens is not modified by any of them, so every repetition writes the
same rows.

An eager launch through Python and ctypes costs some 15 us, which hides a kernel shorter than that: with --graph each side is also
captured as a HIP graph of 20 calls and the replay timed (`*_graph` fields, microseconds a call), as benchmarks/tiny_grid.py does."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "decode", "bench_append_varlen.jsonl")
H_KV, D, HELD = 8, 128, 4096
GRAPH_CALLS = 20

SHAPES = {  # name: (tokens a sequence, page_size (0: contiguous), fp8 cache)
    "a": ([512] * 4, 0, False),
    "b": ([1024] + [1] * 63, 0, False),
    "c": ([1] * 64, 0, False),
    "d": ([512] * 4, 256, False),
    "e": ([512] * 4, 0, True),
}


class Shape:
    def __init__(self, name, dev):
        import torch
        from flash_attention_dlrs_amd import _lib
        from flash_attention_dlrs_amd.flash_attention_torch import convert_triton_dtype
        self.torch, self._lib, self.name = torch, _lib, name
        self.n_new, self.page, fp8 = SHAPES[name]
        B, total = len(self.n_new), sum(self.n_new)
        cap = HELD + -(-max(self.n_new) // 256) * 256  # room for the longest chunk, a whole number of 256-key pages
        bf = torch.bfloat16
        mk = lambda *sh: (torch.randn(*sh, device=dev) * 0.8).to(bf)  # noqa: E731
        self.k_new, self.v_new = mk(total, H_KV, D), mk(total, H_KV, D)
        kv = torch.float8_e4m3fn if fp8 else bf
        self.table = None
        if self.page:
            mb = cap // self.page
            self.K, self.V = mk(B * mb, H_KV, self.page, D), mk(B * mb, H_KV, self.page, D)
            self.table = torch.randperm(B * mb, device=dev).to(torch.int32).view(B, mb)
        else:
            self.K, self.V = mk(B, H_KV, cap, D).to(kv), mk(B, H_KV, cap, D).to(kv)
        self.kd = self.vd = None
        if fp8:
            self.kd, self.vd = (torch.rand(B, H_KV, device=dev) * 0.01 + 0.005 for _ in range(2))
        ang = torch.rand(cap, D // 2, device=dev, dtype=torch.float64) * 6.283
        self.cos, self.sin = ang.cos().to(bf), ang.sin().to(bf)
        self.lens = torch.full((B,), HELD, dtype=torch.int32, device=dev)
        self.out = torch.empty_like(self.lens)
        self.cu = torch.tensor([0] + self.n_new, dtype=torch.int64).cumsum(0).to(torch.int32).to(dev)
        self.enum, self.kv_enum = convert_triton_dtype(bf), convert_triton_dtype(kv)
        self.info = dict(B=B, H_kv=H_KV, d=D, total_new=total, max_seqlen_new=max(self.n_new), held=HELD, capacity=cap,
                         page_size=self.page, kv_dtype="e4m3" if fp8 else "bf16",
                         moved_bytes=total * H_KV * D * 2 * (2 + (1 if fp8 else 2)))  # K and V rows read and written
        # the groups of equal length: (first sequence, sequences, tokens each, first packed row); consecutive in these shapes
        self.groups, b, row = [], 0, 0
        while b < B:
            e = b
            while e < B and self.n_new[e] == self.n_new[b]:
                e += 1
            self.groups.append((b, e - b, self.n_new[b], row))
            row += (e - b) * self.n_new[b]
            b = e

    def packed(self):
        def run():
            self._lib.fa2_kvcache_append_varlen(self.K, self.V, self.k_new, self.v_new, self.cu, self.info["max_seqlen_new"], self.lens,
                                                self.out, self.enum, self.kv_enum, block_table=self.table, k_descale=self.kd,
                                                v_descale=self.vd, rotary_cos=self.cos, rotary_sin=self.sin)
        return run

    def _fixed_call(self, b0, nb, n, row):
        """The arguments of one fa2_kvcache_append for sequences [b0, b0 + nb) at n tokens each: views, made once."""
        rows = slice(b0, b0 + nb)
        kn, vn = (t[row:row + nb * n].view(nb, n, H_KV, D).transpose(1, 2) for t in (self.k_new, self.v_new))
        K, V = (self.K, self.V) if self.page else (self.K[rows], self.V[rows])
        kw = dict(block_table=None if self.table is None else self.table[rows], k_descale=None if self.kd is None else self.kd[rows],
                  v_descale=None if self.vd is None else self.vd[rows], rotary_cos=self.cos, rotary_sin=self.sin)
        return (K, V, kn, vn, self.lens[rows], self.out[rows], self.enum, self.kv_enum), kw

    def grouped(self):
        calls = [self._fixed_call(*g) for g in self.groups]

        def run():
            for a, kw in calls:
                self._lib.fa2_kvcache_append(*a, **kw)
        return run

    def fixed(self):
        a, kw = self._fixed_call(0, len(self.n_new), self.n_new[0], 0)
        return lambda: self._lib.fa2_kvcache_append(*a, **kw)


def time_us(torch, fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def interleaved(torch, fns, iters, rounds, per_call=1):
    for f in fns:
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(rounds):
        for k, f in enumerate(fns):
            ts[k].append(time_us(torch, f, iters) / per_call)
    return [dict(median_us=round(sorted(t)[len(t) // 2], 2), min_us=round(min(t), 2), max_us=round(max(t), 2)) for t in ts]


def graphs_of(torch, fns):
    """Each side as a replayable HIP graph of GRAPH_CALLS calls."""
    out = []
    for f in fns:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(GRAPH_CALLS):
                f()
        out.append(g.replay)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--graph", action="store_true", help="also time each side as a HIP graph of %d calls" % GRAPH_CALLS)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fh:
        for name in args.shapes.split(","):
            s = Shape(name, dev)
            sides = {"packed": s.packed(), "grouped": s.grouped()}
            if name == "c":
                sides["fixed"] = s.fixed()
            rec = dict(kind="events_append_varlen", shape=name, **s.info, groups=len(s.groups), iters=args.iters, rounds=args.rounds)
            rec.update(zip(sides, interleaved(torch, list(sides.values()), args.iters, args.rounds)))
            if args.graph:
                replays = graphs_of(torch, list(sides.values()))
                res = interleaved(torch, replays, max(args.iters // 5, 4), args.rounds, GRAPH_CALLS)
                rec.update({k + "_graph": r for k, r in zip(sides, res)})
            line = json.dumps(rec)
            print(line, flush=True)
            fh.write(line + "\n")
            fh.flush()
            del s
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
