#!/usr/bin/env python3
"""KV-cache decode attention timing (fa2_fwd_kvcache, fa2_fwd_kvcache_fp8), bf16; JSON lines appended to profiles/decode/bench_decode.jsonl.

Sides, alternated in one process after every shape has been warmed:
  decode: flash_attention_kvcache_forward, AUTO variant and auto num_splits;
  varlen: the route without this entry point -- flash_attention_varlen_forward with N_q tokens per sequence on the packed
          cache (equal lengths: the (B, S, H_kv, d) cache viewed as (B S, H_kv, d); the ragged case packs the real lengths);
  sdpa:   torch scaled_dot_product_attention with enable_gqa (the ragged case with a boolean key mask).
Every side rotates over enough copies of K and V to exceed the 256 MiB last-level cache, so the keys come from HBM.

Records:
  kind=events   call time from device events around `iters` back-to-back calls, median / min / max over `rounds` (this includes
                what the host takes to enqueue a call: at these sizes the host often is the limit, for every side);
  kind=kernels  kernel time per call from a `rocprofv3 --kernel-trace --stats` run of its own (a fresh child process per shape,
                --rocprof), average / min / max / stddev as the stats file gives them, and K + V bytes over the decode kernel time
                as a share of the 6.29 TB/s copy rate of the chip;
  kind=sweep    the events figure of the decode side for num_splits in {1, 2, 4, 8, 16, 32, 64} on the first four shapes (--sweep);
  kind=sweep_kernels  the same sweep in kernel time (--rocprof DIR --sweep): one traced child per shape runs the split counts one
                after the other, and the dispatches of the kernel trace are cut into the split counts by their order (split kernel
                plus combine per call; one kernel for num_splits = 1).

--kv-dtype e4m3 | e5m2 adds the fp8-cache decode (fa2_fwd_kvcache_fp8; the same K and V through quantize_kv_cache, per-(b, h_kv)
descales) as one more side, decode_fp8, alternated with the others in the same process; records go to bench_decode_fp8.jsonl.
The combine kernel is common to the two decode sides, so kind=kernels is then read off the kernel trace (each combine belongs
to the split kernel in front of it; the first 3 calls of a side are its warm-up) instead of the stats file; fp8_over_16 is the
ratio of the two decode averages and hbm_share_fp8 counts the fp8 bytes.  The sweeps then run the fp8 side.

--page-size N times the paged decode (fa2_fwd_kvcache_paged) against the contiguous call of the same build on the same shapes: K
and V of every copy are scattered into a (num_blocks, N, H_kv, d) pool under a random permutation table, and the sides are
decode, decode_paged and gather (the route the paged call replaces: index_select of every sequence's pages into a padded cache,
then the contiguous decode).  kind=events times all three; with --rocprof the traced child alternates decode and decode_paged
alone and kind=kernels_paged is read off the kernel trace as in the fp8 mode (paged_over_contiguous is the ratio of the two
averages).  Records go to bench_decode.jsonl.

--append times the decode step with its cache update (fa2_fwd_kvcache_append), by device events, N_new = 1: the sides are fused
(the one call), torch (the route it replaces: apply_rotary on Q and K, the quantisation with the given descales where the cache
is fp8, an index_put through the block table where it is paged, then the existing decode call with the bumped lengths) and decode
(the existing call alone, for the cost of the step beyond it).  It goes with --kv-dtype and --page-size, which then choose the
cache.  A last record, case prefill_append, times kvcache_append alone against the torch route at N_new = 2048, B 8, H_kv 8,
d 128 (K plus V 64 MiB): hbm_share counts the bytes read plus the bytes written (2 x 64 MiB, plus the tables) over the copy rate.
Records: kind=events_append, bench_decode.jsonl."""
import argparse
import csv
import glob
import json
import math
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "decode", "bench_decode.jsonl")
OUT_FP8 = os.path.join(ROOT, "profiles", "decode", "bench_decode_fp8.jsonl")
KV_DTYPES = ("same", "e4m3", "e5m2")
HBM_COPY_RATE = 6.29e12  # bytes / s, measured copy rate of the MI355X

CASES = {  # name: (B, H, H_kv, N_k, d, N_q)
    "b1_n8192": (1, 32, 8, 8192, 128, 1),
    "b1_n131072": (1, 32, 8, 131072, 128, 1),
    "b4_n8192": (4, 32, 8, 8192, 128, 1),
    "b16_n4096": (16, 32, 8, 4096, 128, 1),
    "b64_n2048": (64, 32, 8, 2048, 128, 1),
    "mha_b8_n4096": (8, 32, 32, 4096, 128, 1),
    "mqa_b8_n4096": (8, 32, 1, 4096, 128, 1),
    "d64_b4_n8192": (4, 32, 8, 8192, 64, 1),
    "nq4_b4_n8192": (4, 32, 8, 8192, 128, 4),
    "ragged_b16": (16, 32, 8, 16384, 128, 1),  # lengths from 100 to 16384
}
SWEEP_CASES = ("b1_n8192", "b1_n131072", "b4_n8192", "b16_n4096")
SWEEP_SPLITS = (1, 2, 4, 8, 16, 32, 64)


def emit(fh, **kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if fh is not None:
        fh.write(line + "\n")
        fh.flush()


def ragged_lengths(B, lo, hi):
    return [int(round(math.exp(math.log(lo) + (math.log(hi) - math.log(lo)) * k / (B - 1)))) for k in range(B)]


class Case:
    def __init__(self, name, dev, kv_dtype="same", page_size=0):
        import torch
        from flash_attention_dlrs_amd import _lib
        from flash_attention_dlrs_amd.flash_attention_torch import convert_triton_dtype
        self.torch, self._lib, self.name, self.dev = torch, _lib, name, dev
        B, H, H_kv, S, d, N_q = CASES[name]
        self.shape = dict(B=B, H=H, H_kv=H_kv, N_k=S, d=d, N_q=N_q)
        self.lens = ragged_lengths(B, 100, S) if name.startswith("ragged") else [S] * B
        self.kv_bytes = 2 * 2 * H_kv * d * sum(self.lens)
        self.copies = max(2, min(16, math.ceil(600e6 / (2 * 2 * B * H_kv * S * d))))
        self.scale = d ** -0.5
        self.enum = convert_triton_dtype(torch.bfloat16)
        mk = lambda *s: (torch.randn(*s, device=dev) * 0.8).to(torch.bfloat16)  # noqa: E731
        self.Q = mk(B, H, N_q, d)
        self.K = [mk(B, S, H_kv, d) for _ in range(self.copies)]  # the flash-attn cache layout
        self.V = [mk(B, S, H_kv, d) for _ in range(self.copies)]
        self.lens_dev = torch.tensor(self.lens, dtype=torch.int32, device=dev)
        self.ragged = len(set(self.lens)) > 1
        # varlen side: packed keys, N_q query tokens per sequence
        self.Qp = self.Q.transpose(1, 2).reshape(B * N_q, H, d).contiguous()
        self.cu_q = torch.arange(0, (B + 1) * N_q, N_q, dtype=torch.int32, device=dev)
        self.cu_k = torch.tensor([0] + list(torch.tensor(self.lens).cumsum(0).tolist()), dtype=torch.int32, device=dev)
        if self.ragged:
            pk = lambda t: torch.cat([t[b, :n] for b, n in enumerate(self.lens)])  # noqa: E731
            self.Kp, self.Vp = [pk(t) for t in self.K], [pk(t) for t in self.V]
            self.mask = (torch.arange(S, device=dev).view(1, 1, 1, S) < self.lens_dev.view(B, 1, 1, 1))
        else:
            self.Kp, self.Vp = [t.view(B * S, H_kv, d) for t in self.K], [t.view(B * S, H_kv, d) for t in self.V]
            self.mask = None
        self.O = torch.empty(B, H, N_q, d, dtype=torch.bfloat16, device=dev)
        self.L = torch.empty(B, H, N_q, dtype=torch.bfloat16, device=dev)
        self.i = 0
        self.kv_dtype = kv_dtype
        if kv_dtype != "same":  # the same caches in fp8, (B, S, H_kv, d) storage as well
            from flash_attention_dlrs_amd import quantize_kv_cache
            fmt = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}[kv_dtype]
            self.kv_enum = convert_triton_dtype(fmt)
            self.kv8_bytes = self.kv_bytes // 2

            def q8(t):
                t8, ds = quantize_kv_cache(t.transpose(1, 2), fmt)
                return t8.view(torch.uint8).transpose(1, 2).contiguous().view(fmt), ds
            self.K8, self.V8 = [q8(t) for t in self.K], [q8(t) for t in self.V]
        self.page_size = page_size
        if page_size:  # every copy scattered into a flash-attn-layout pool (num_blocks, P, H_kv, d) under one random table
            assert S % page_size == 0, (S, page_size)
            mb = S // page_size
            perm = torch.randperm(B * mb, generator=torch.Generator().manual_seed(0)).to(dev)
            self.table = perm.view(B, mb).to(torch.int32)
            self.pages = perm  # index_select argument of the gather route

            def pool(t):
                p = torch.empty(B * mb, page_size, H_kv, d, dtype=t.dtype, device=dev)
                p[perm] = t.view(B * mb, page_size, H_kv, d)
                return p
            self.K_pool, self.V_pool = [pool(t) for t in self.K], [pool(t) for t in self.V]

    def auto_splits(self):
        s = self.shape
        return self._lib.kvcache_num_splits(s["B"], s["H"], s["H_kv"], s["N_q"], s["N_k"], s["d"], self.enum)

    def decode(self, num_splits=0):
        """The library launch itself, outputs and workspace allocated once (what a serving loop does)."""
        s = self.shape
        n = num_splits or self.auto_splits()
        words = self._lib.kvcache_workspace_bytes(s["B"], s["H"], s["N_q"], s["d"], n) // 4
        ws = self.torch.empty(max(words, 1), dtype=self.torch.float32, device=self.dev)

        def run():
            self.i = (self.i + 1) % self.copies
            self._lib.fa2_fwd_kvcache(self.Q, self.K[self.i].transpose(1, 2), self.V[self.i].transpose(1, 2), self.O, self.L,
                                      self.lens_dev, self.enum, scale=self.scale, num_splits=n, workspace=ws)
        return run

    def decode_fp8(self, num_splits=0):
        """The fp8-cache launch, under the same conditions."""
        s = self.shape
        n = num_splits or self.auto_splits()
        words = self._lib.kvcache_workspace_bytes(s["B"], s["H"], s["N_q"], s["d"], n) // 4
        ws = self.torch.empty(max(words, 1), dtype=self.torch.float32, device=self.dev)

        def run():
            self.i = (self.i + 1) % self.copies
            (K8, kd), (V8, vd) = self.K8[self.i], self.V8[self.i]
            self._lib.fa2_fwd_kvcache_fp8(self.Q, K8.transpose(1, 2), V8.transpose(1, 2), self.O, self.L, self.lens_dev, self.enum,
                                          self.kv_enum, k_descale=kd, v_descale=vd, scale=self.scale, num_splits=n, workspace=ws)
        return run

    def decode_paged(self, num_splits=0):
        """The paged launch over the pools, under the same conditions."""
        s = self.shape
        n = num_splits or self.auto_splits()
        words = self._lib.kvcache_workspace_bytes(s["B"], s["H"], s["N_q"], s["d"], n) // 4
        ws = self.torch.empty(max(words, 1), dtype=self.torch.float32, device=self.dev)

        def run():
            self.i = (self.i + 1) % self.copies
            self._lib.fa2_fwd_kvcache_paged(self.Q, self.K_pool[self.i].transpose(1, 2), self.V_pool[self.i].transpose(1, 2), self.O,
                                            self.L, self.table, self.lens_dev, self.enum, self.enum, scale=self.scale, num_splits=n,
                                            workspace=ws)
        return run

    def gather(self):
        """The route the paged call replaces: gather every sequence's pages into a padded cache, then the contiguous decode."""
        s = self.shape
        n = self.auto_splits()
        words = self._lib.kvcache_workspace_bytes(s["B"], s["H"], s["N_q"], s["d"], n) // 4
        ws = self.torch.empty(max(words, 1), dtype=self.torch.float32, device=self.dev)
        shape = (s["B"], s["N_k"], s["H_kv"], s["d"])

        def run():
            self.i = (self.i + 1) % self.copies
            K = self.torch.index_select(self.K_pool[self.i], 0, self.pages).view(shape)
            V = self.torch.index_select(self.V_pool[self.i], 0, self.pages).view(shape)
            self._lib.fa2_fwd_kvcache(self.Q, K.transpose(1, 2), V.transpose(1, 2), self.O, self.L, self.lens_dev, self.enum,
                                      scale=self.scale, num_splits=n, workspace=ws)
        return run

    def varlen(self):
        from flash_attention_dlrs_amd import flash_attention_varlen_forward
        s = self.shape

        def run():
            self.i = (self.i + 1) % self.copies
            flash_attention_varlen_forward(self.Qp, self.Kp[self.i], self.Vp[self.i], self.cu_q, self.cu_k, s["N_q"], max(self.lens),
                                           self.dev, scale=self.scale)
        return run

    def sdpa(self):
        F = self.torch.nn.functional

        def run():
            self.i = (self.i + 1) % self.copies
            F.scaled_dot_product_attention(self.Q, self.K[self.i].transpose(1, 2), self.V[self.i].transpose(1, 2),
                                           attn_mask=self.mask, scale=self.scale, enable_gqa=True)
        return run

    def append_setup(self):
        """The decode step's inputs: one new token per sequence in flash-attn's (B, 1, H_kv, d) storage, rotary tables, and lengths
        one short of the case's, so that the attention after the append is the case's."""
        torch = self.torch
        s, dev = self.shape, self.dev
        mk = lambda *sh: (torch.randn(*sh, device=dev) * 0.8).to(torch.bfloat16)  # noqa: E731
        self.k_new, self.v_new = mk(s["B"], 1, s["H_kv"], s["d"]).transpose(1, 2), mk(s["B"], 1, s["H_kv"], s["d"]).transpose(1, 2)
        ang = torch.rand(s["N_k"] + 8, s["d"] // 2, device=dev, dtype=torch.float64) * 6.283
        self.cos, self.sin = ang.cos().to(torch.bfloat16), ang.sin().to(torch.bfloat16)
        self.lens_before = self.lens_dev - 1
        self.lens_out = torch.empty_like(self.lens_dev)
        self.q_rot = torch.empty_like(self.Q)
        fp8 = self.kv_dtype != "same"
        self.cache_enum = self.kv_enum if fp8 else self.enum
        if self.page_size:  # pools in the cache's dtype
            if fp8:
                P, perm = self.page_size, self.pages
                pool8 = lambda t8: t8.view(torch.uint8).view(-1, P, s["H_kv"], s["d"])[torch.argsort(perm)].view(t8.dtype)  # noqa: E731
                self.cK, self.cV = [pool8(k8) for k8, _ in self.K8], [pool8(v8) for v8, _ in self.V8]
            else:
                self.cK, self.cV = self.K_pool, self.V_pool
        else:
            self.cK, self.cV = ([k8 for k8, _ in self.K8], [v8 for v8, _ in self.V8]) if fp8 else (self.K, self.V)
        self.kds = [kd for _, kd in self.K8] if fp8 else [None] * self.copies
        self.vds = [vd for _, vd in self.V8] if fp8 else [None] * self.copies
        n = self.auto_splits()
        words = self._lib.kvcache_workspace_bytes(s["B"], s["H"], s["N_q"], s["d"], n) // 4
        self.append_ws, self.append_n = torch.empty(max(words, 1), dtype=torch.float32, device=dev), n

    def decode_any(self, Q, lens):
        """The existing decode call over copy self.i of whichever cache --kv-dtype and --page-size chose."""
        i = self.i
        K, V = self.cK[i].transpose(1, 2), self.cV[i].transpose(1, 2)
        kw = dict(scale=self.scale, num_splits=self.append_n, workspace=self.append_ws)
        if self.page_size:
            self._lib.fa2_fwd_kvcache_paged(Q, K, V, self.O, self.L, self.table, lens, self.enum, self.cache_enum,
                                            k_descale=self.kds[i], v_descale=self.vds[i], **kw)
        elif self.kv_dtype != "same":
            self._lib.fa2_fwd_kvcache_fp8(Q, K, V, self.O, self.L, lens, self.enum, self.cache_enum, k_descale=self.kds[i],
                                          v_descale=self.vds[i], **kw)
        else:
            self._lib.fa2_fwd_kvcache(Q, K, V, self.O, self.L, lens, self.enum, **kw)

    def append_decode_alone(self):
        def run():
            self.i = (self.i + 1) % self.copies
            self.decode_any(self.Q, self.lens_dev)
        return run

    def append_fused(self):
        def run():
            self.i = i = (self.i + 1) % self.copies
            self._lib.fa2_fwd_kvcache_append(self.Q, self.cK[i].transpose(1, 2), self.cV[i].transpose(1, 2), self.O, self.L, self.k_new,
                                             self.v_new, self.lens_before, self.lens_out, self.enum, self.cache_enum,
                                             block_table=self.table if self.page_size else None, k_descale=self.kds[i],
                                             v_descale=self.vds[i], rotary_cos=self.cos, rotary_sin=self.sin, q_rot=self.q_rot,
                                             scale=self.scale, num_splits=self.append_n, workspace=self.append_ws)
        return run

    def append_torch(self):
        """The route the fused call replaces, as an engine would write it in torch."""
        from flash_attention_dlrs_amd import apply_rotary
        torch = self.torch
        rows = torch.arange(self.shape["B"], device=self.dev)

        def run():
            self.i = i = (self.i + 1) % self.copies
            pos = self.lens_before.long()
            q = apply_rotary(self.Q, self.cos, self.sin, pos[:, None, None])
            k = apply_rotary(self.k_new, self.cos, self.sin, pos[:, None, None])[:, :, 0]
            v = self.v_new[:, :, 0]
            if self.kv_dtype != "same":
                top = torch.finfo(self.cK[i].dtype).max
                k = (k.float() / self.kds[i][:, :, None]).clamp(-top, top).to(self.cK[i].dtype)
                v = (v.float() / self.vds[i][:, :, None]).clamp(-top, top).to(self.cV[i].dtype)
            if self.page_size:
                at = (self.table[rows, pos // self.page_size].long(), pos % self.page_size)
            else:
                at = (rows, pos)
            # (index_put is not implemented for fp8 tensors: the bytes go through a uint8 view)
            raw = (lambda t: t.view(torch.uint8)) if self.kv_dtype != "same" else (lambda t: t)  # noqa: E731
            raw(self.cK[i])[at] = raw(k)
            raw(self.cV[i])[at] = raw(v)
            self.decode_any(q, self.lens_before + 1)
        return run


class PrefillAppend:
    """kvcache_append alone at a prefill size against the torch route: N_new tokens a sequence into an empty cache."""

    def __init__(self, dev, B=8, H_kv=8, N_new=2048, d=128, copies=4):
        import torch
        self.torch, self.shape, self.copies, self.i = torch, dict(B=B, H_kv=H_kv, N_new=N_new, d=d), copies, 0
        mk = lambda *sh: (torch.randn(*sh, device=dev) * 0.8).to(torch.bfloat16)  # noqa: E731
        self.k_new, self.v_new = [mk(B, H_kv, N_new, d) for _ in range(copies)], [mk(B, H_kv, N_new, d) for _ in range(copies)]
        self.K, self.V = [mk(B, H_kv, N_new, d) for _ in range(copies)], [mk(B, H_kv, N_new, d) for _ in range(copies)]
        ang = torch.rand(N_new, d // 2, device=dev, dtype=torch.float64) * 6.283
        self.cos, self.sin = ang.cos().to(torch.bfloat16), ang.sin().to(torch.bfloat16)
        self.lens = torch.zeros(B, dtype=torch.int32, device=dev)
        self.moved_bytes = 2 * 2 * 2 * B * H_kv * N_new * d + 2 * 2 * N_new * (d // 2)  # K and V read and written, the tables read

    def fused(self):
        from flash_attention_dlrs_amd import kvcache_append

        def run():
            self.i = i = (self.i + 1) % self.copies
            kvcache_append(self.K[i], self.V[i], self.k_new[i], self.v_new[i], self.lens, rotary_cos=self.cos, rotary_sin=self.sin)
        return run

    def torch_route(self):
        from flash_attention_dlrs_amd import apply_rotary
        torch, s = self.torch, self.shape
        rows = torch.arange(s["B"], device=self.lens.device)[:, None]
        steps = torch.arange(s["N_new"], device=self.lens.device)

        def run():
            self.i = i = (self.i + 1) % self.copies
            pos = self.lens.long()[:, None] + steps  # (B, N_new): the lengths live on the device
            k = apply_rotary(self.k_new[i], self.cos, self.sin, pos[:, None, :])
            self.K[i].transpose(1, 2)[rows, pos] = k.transpose(1, 2)
            self.V[i].transpose(1, 2)[rows, pos] = self.v_new[i].transpose(1, 2)
            return self.lens + s["N_new"]
        return run


def run_append(names, args, fh):
    import torch
    dev = torch.device("cuda:0")
    for name in names:
        c = Case(name, dev, args.kv_dtype, args.page_size)
        c.append_setup()
        sides = {"fused": c.append_fused(), "torch": c.append_torch(), "decode": c.append_decode_alone()}
        res = interleaved(torch, list(sides.values()), args.iters, args.rounds)
        emit(fh, kind="events_append", case=name, kv_dtype=args.kv_dtype, page_size=args.page_size, N_new=1, **c.shape, ragged=c.ragged,
             num_splits=c.auto_splits(), **{k: r for k, r in zip(sides, res)})
        del c
        torch.cuda.empty_cache()
    p = PrefillAppend(dev)
    sides = {"fused": p.fused(), "torch": p.torch_route()}
    res = interleaved(torch, list(sides.values()), max(args.iters // 5, 4), args.rounds)
    emit(fh, kind="events_append", case="prefill_append", kv_dtype="same", page_size=0, **p.shape, moved_bytes=p.moved_bytes,
         hbm_share=round(p.moved_bytes / (res[0]["median_us"] * 1e-6) / HBM_COPY_RATE, 3), **{k: r for k, r in zip(sides, res)})


def time_us(torch, fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def interleaved(torch, fns, iters, rounds):
    for f in fns:
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(rounds):
        for k, f in enumerate(fns):
            ts[k].append(time_us(torch, f, iters))
    return [dict(median_us=round(sorted(t)[len(t) // 2], 2), min_us=round(min(t), 2), max_us=round(max(t), 2)) for t in ts]


def run_events(names, args, fh):
    import torch
    dev = torch.device("cuda:0")
    for name in names:
        c = Case(name, dev, args.kv_dtype, args.page_size)
        if args.page_size:
            sides = {"decode": c.decode(), "decode_paged": c.decode_paged(), "gather": c.gather()}
            res = interleaved(torch, list(sides.values()), args.iters, args.rounds)
            emit(fh, kind="events_paged", case=name, page_size=args.page_size, **c.shape, ragged=c.ragged, num_splits=c.auto_splits(),
                 kv_bytes=c.kv_bytes, **{k: r for k, r in zip(sides, res)})
            del c
            torch.cuda.empty_cache()
            continue
        sides = {"decode": c.decode(), "varlen": c.varlen()}
        if args.kv_dtype != "same":
            sides["decode_fp8"] = c.decode_fp8()
        if not args.no_sdpa:
            sides["sdpa"] = c.sdpa()
        res = interleaved(torch, list(sides.values()), args.iters, args.rounds)
        emit(fh, kind="events", case=name, **c.shape, ragged=c.ragged, num_splits=c.auto_splits(), kv_bytes=c.kv_bytes,
             **{k: r for k, r in zip(sides, res)})
        if args.sweep and name in SWEEP_CASES:
            fns = [(c.decode if args.kv_dtype == "same" else c.decode_fp8)(n) for n in SWEEP_SPLITS]
            for n, r in zip(SWEEP_SPLITS, interleaved(torch, fns, args.iters, args.rounds)):
                emit(fh, kind="sweep", case=name, kv_dtype=args.kv_dtype, **c.shape, num_splits=n, **r)
        del c
        torch.cuda.empty_cache()


def run_pass(name, args):
    """The traced child: warm, then alternate the sides; the profiler's stats file holds the kernel times."""
    import torch
    c = Case(name, torch.device("cuda:0"), args.kv_dtype, args.page_size)
    if args.page_size:  # the paged call against the contiguous one, nothing else
        sides = [c.decode(), c.decode_paged()]
    else:
        sides = [c.decode()] + ([] if args.kv_dtype == "same" else [c.decode_fp8()]) + [c.varlen()] + ([] if args.no_sdpa else [c.sdpa()])
    for _ in range(args.iters + 3):
        for f in sides:
            f()
    torch.cuda.synchronize()
    extra = {} if args.kv_dtype == "same" else dict(kv_dtype=args.kv_dtype, kv8_bytes=c.kv8_bytes)
    if args.page_size:
        extra["page_size"] = args.page_size
    print(json.dumps(dict(case=name, calls=args.iters + 3, kv_bytes=c.kv_bytes, num_splits=c.auto_splits(), **extra, **c.shape)))


def run_sweep_pass(name, args):
    """The traced child of the kernel-time sweep: the decode side alone, one split count after the other."""
    import torch
    c = Case(name, torch.device("cuda:0"), args.kv_dtype)
    for n in SWEEP_SPLITS:
        f = c.decode(n) if args.kv_dtype == "same" else c.decode_fp8(n)
        for _ in range(args.iters + 3):
            f()
        torch.cuda.synchronize()
    kv = dict(kv_bytes=c.kv_bytes) if args.kv_dtype == "same" else dict(kv_bytes=c.kv8_bytes, kv_dtype=args.kv_dtype)
    print(json.dumps(dict(case=name, calls=args.iters + 3, auto_splits=c.auto_splits(), **kv, **c.shape)))


def traced_child(out, extra, args):
    os.makedirs(out, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable,
           os.path.abspath(__file__), "--iters", str(args.iters), "--kv-dtype", args.kv_dtype, "--page-size", str(args.page_size)] + \
        extra + \
        (["--no-sdpa"] if args.no_sdpa else [])
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.child_timeout)
    if p.returncode != 0:  # a failed child ends the run: nothing more is started on the GPU
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
        sys.exit(p.returncode)
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def sweep_from_trace(out, info, fh):
    trace = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
    rows = [r for r in csv.DictReader(open(trace[0])) if "fa2_decode" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    pos, calls = 0, info["calls"]
    for n in SWEEP_SPLITS:
        per = 1 if n == 1 else 2
        seg = rows[pos:pos + per * calls]
        pos += per * calls
        assert len(seg) == per * calls and all(("combine" in r["Kernel_Name"]) == (per == 2 and k % 2 == 1) for k, r in enumerate(seg)), n
        us = [sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in seg[per * k:per * k + per]) / 1e3 for k in range(3, calls)]
        avg = sum(us) / len(us)
        emit(fh, kind="sweep_kernels", case=info["case"], kv_dtype=info.get("kv_dtype", "same"), num_splits=n, auto_splits=info["auto_splits"], avg_us=round(avg, 2),
             min_us=round(min(us), 2), max_us=round(max(us), 2),
             hbm_share=round(info["kv_bytes"] / (avg * 1e-6) / HBM_COPY_RATE, 3))
    assert pos == len(rows)


PAGED_KERNEL = re.compile(r"fa2_decode_\w+_kernel<[^>]*\btrue\b")  # the PAGED template argument of the split kernels


def side_of(kernel):
    if "fa2_decode" in kernel:  # (the combine kernel, common to the decode sides, counts as "decode" here)
        if PAGED_KERNEL.search(kernel):
            return "decode_paged"
        return "decode_fp8" if "Cache" in kernel else "decode"
    if "varlen" in kernel:
        return "varlen"
    low = kernel.lower()
    if "attn" in low or "fmha" in low or "attention" in low:
        return "sdpa"
    return None


def sides_from_trace(out, info):
    """Per-call kernel time of every side from the kernel trace, in dispatch order: a decode combine belongs to the split kernel
    in front of it.  The first 3 calls of a side are its warm-up."""
    trace = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
    rows = sorted(csv.DictReader(open(trace[0])), key=lambda r: int(r["Start_Timestamp"]))
    per_side, last = {}, None
    for r in rows:
        side = side_of(r["Kernel_Name"])
        if side is None:
            continue
        if "combine" in r["Kernel_Name"] and "fa2_decode" in r["Kernel_Name"]:
            side = last
        elif side.startswith("decode"):
            last = side
        per_side.setdefault(side, []).append(r)
    sides = {}
    for side, rs in per_side.items():
        per, calls = len(rs) // info["calls"], info["calls"]
        if per * calls != len(rs) and not side.startswith("decode"):
            continue  # a side whose launches per call vary (torch's choice) has no per-call figure here
        assert per >= 1 and per * calls == len(rs), (side, len(rs), calls)
        us = [sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rs[per * k:per * k + per]) / 1e3 for k in range(3, calls)]
        avg = sum(us) / len(us)
        sides[side] = dict(avg_us=round(avg, 2), min_us=round(min(us), 2), max_us=round(max(us), 2),
                           stddev_us=round((sum((u - avg) ** 2 for u in us) / len(us)) ** 0.5, 2),
                           kernels=sorted({r["Kernel_Name"][:90] for r in rs}))
    return sides


def run_rocprof(names, args, fh):
    for name in names:
        out = os.path.join(args.rocprof, name)
        info = traced_child(out, ["--pass-case", name], args)
        if args.page_size:
            sides = sides_from_trace(out, info)
            flat, paged = sides["decode"]["avg_us"], sides["decode_paged"]["avg_us"]
            emit(fh, kind="kernels_paged", **info, hbm_share=round(info["kv_bytes"] / (flat * 1e-6) / HBM_COPY_RATE, 3),
                 hbm_share_paged=round(info["kv_bytes"] / (paged * 1e-6) / HBM_COPY_RATE, 3),
                 paged_over_contiguous=round(paged / flat, 3), **sides)
            continue
        if args.kv_dtype != "same":
            sides = sides_from_trace(out, info)
            d16, d8 = sides["decode"]["avg_us"], sides["decode_fp8"]["avg_us"]
            emit(fh, kind="kernels", **info, hbm_share=round(info["kv_bytes"] / (d16 * 1e-6) / HBM_COPY_RATE, 3),
                 hbm_share_fp8=round(info["kv8_bytes"] / (d8 * 1e-6) / HBM_COPY_RATE, 3), fp8_over_16=round(d8 / d16, 3), **sides)
            if args.sweep and name in SWEEP_CASES:
                out = os.path.join(args.rocprof, name + "_sweep")
                sweep_from_trace(out, traced_child(out, ["--sweep-case", name], args), fh)
            continue
        stats = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
        sides = {}
        for row in csv.DictReader(open(stats[0])):
            side = side_of(row["Name"])
            if side is None:
                continue
            s = sides.setdefault(side, dict(avg_us=0.0, min_us=0.0, max_us=0.0, stddev_us=0.0, kernels=[]))
            per_call = int(row["Calls"]) / info["calls"]  # launches of this kernel per call of the side
            s["avg_us"] += float(row["AverageNs"]) * per_call / 1e3
            s["min_us"] += float(row["MinNs"]) * per_call / 1e3
            s["max_us"] += float(row["MaxNs"]) * per_call / 1e3
            s["stddev_us"] += float(row["StdDev"]) * per_call / 1e3
            s["kernels"].append("%s x%g avg %.2f us" % (row["Name"][:90], per_call, float(row["AverageNs"]) / 1e3))
        for s in sides.values():
            for k in ("avg_us", "min_us", "max_us", "stddev_us"):
                s[k] = round(s[k], 2)
        share = info["kv_bytes"] / (sides["decode"]["avg_us"] * 1e-6) / HBM_COPY_RATE if "decode" in sides else None
        emit(fh, kind="kernels", **info, hbm_share=None if share is None else round(share, 3), **sides)
        if args.sweep and name in SWEEP_CASES:
            out = os.path.join(args.rocprof, name + "_sweep")
            sweep_from_trace(out, traced_child(out, ["--sweep-case", name], args), fh)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sweep", action="store_true", help="also time num_splits in %s on the first four shapes" % (SWEEP_SPLITS,))
    ap.add_argument("--no-sdpa", action="store_true")
    ap.add_argument("--rocprof", metavar="DIR", help="kernel times: one rocprofv3 --kernel-trace --stats child per shape, traces under DIR")
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--pass-case", help=argparse.SUPPRESS)
    ap.add_argument("--sweep-case", help=argparse.SUPPRESS)
    ap.add_argument("--kv-dtype", choices=KV_DTYPES, default="same", help="also time the decode over an fp8 cache of this format")
    ap.add_argument("--page-size", type=int, default=0, metavar="N",
                    help="time the paged decode over pools of N-key pages against the contiguous decode (N must divide every N_k)")
    ap.add_argument("--append", action="store_true",
                    help="time the decode step with its cache update (fused call against the torch route), and the prefill-sized append")
    ap.add_argument("--out", help="default: profiles/decode/bench_decode.jsonl, bench_decode_fp8.jsonl with --kv-dtype")
    args = ap.parse_args()
    args.out = args.out or (OUT if args.kv_dtype == "same" or args.append else OUT_FP8)
    if args.append and (args.sweep or args.rocprof):
        ap.error("--append goes without --sweep and --rocprof")
    if args.page_size and not args.append and (args.kv_dtype != "same" or args.sweep):
        ap.error("--page-size goes without --kv-dtype and --sweep")
    if args.pass_case:
        return run_pass(args.pass_case, args)
    if args.sweep_case:
        return run_sweep_pass(args.sweep_case, args)
    names = args.cases.split(",")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fh:
        if args.append:
            run_append(names, args, fh)
        elif args.rocprof:
            run_rocprof(names, args, fh)
        else:
            run_events(names, args, fh)


if __name__ == "__main__":
    main()
