#!/usr/bin/env python3
"""Backward of un-absorbed MLA prefill (fa2_bwd_varlen_dv: d = 192, d_v = 128), bf16, causal, H_kv = H; JSON lines appended to
profiles/mla/bench_mla_prefill_bwd.jsonl.  Protocol, shapes and cache rotation are benchmarks/bench_mla_prefill.py's: kernel times
come from a `rocprofv3 --kernel-trace --stats` child per shape (a fresh process, under its own `timeout -k 10`; the first non-zero
status ends the run), every side rotates over enough copies of K and V to exceed the 256 MiB last-level cache, each side is warmed
(calls not counted) and then run back to back, and avg, min-max and stddev are reported per call (the three launches of a call -- D,
the query owner, the key owner -- summed; `launches` holds the auto side's average per launch).

Sides of one child:
  auto      the call under AUTO (the matrix kernel mfma16dv);
  generic   the same call with the VALU form forced;
  padded    the only route without this entry point: flash_attention_varlen_backward with V, O and dO zero-padded to 192 columns
            (padded once, outside the timed calls); that call pads every head size to 256 and runs the VALU kernel.  Only the
            library's own kernels are counted, not the padding copies the call makes;
  d128      fa2_bwd_varlen at d = 128 on the same lengths (mfma16): the yardstick.  The algorithmic FLOP ratio to it is
            (3 * 192 + 2 * 128) / (5 * 128) = 1.30, the executed one (S and dP are computed by both owners) (4 * 192 + 3 * 128) /
            (7 * 128) = 1.29; auto_over_d128 is the time ratio;
  sdpa      torch autograd through torch.nn.functional.scaled_dot_product_attention, one call per sequence, forward and backward
            kernels together (fused backends first; the math backend only where its score matrix stays below 8 GiB; null with the
            reason where neither runs).
The kernel trace is cut into the library's sides by dispatch order (three backward kernels per call); sdpa's timed calls are the rows
behind the last of them (its warm-up runs first).

TFLOP/s count 2 * visible pairs * H * (3 d + 2 d_v)."""
import argparse
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_mla_decode import emit, per_call, trace_rows  # noqa: E402
from bench_mla_prefill import BATCHES, CASES, D, D_V, visible_pairs  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "mla", "bench_mla_prefill_bwd.jsonl")
PER = 3  # kernels of one backward call: D, the query owner, the key owner
# the library's, by name (the VALU kernels are bwd_main_kernel<E, MODE, F> / bwd_D_kernel<E, F> whatever the form)
OURS = ("bwd_mfma16dv_kernel", "bwd_D_dv_kernel", "bwd_main_kernel", "bwd_D_kernel", "bwd_D_varlen", "bwd_mfma16_varlen")


class Case:
    def __init__(self, name, dev):
        import torch
        import flash_attention_dlrs_amd as fa
        from flash_attention_dlrs_amd import _lib
        from flash_attention_dlrs_amd.flash_attention_torch import convert_triton_dtype
        self.torch, self._lib, self.fa, self.dev = torch, _lib, fa, dev
        batch, H = CASES[name]
        self.lq, self.lk = BATCHES[batch]
        self.H, self.tq, self.tk = H, sum(self.lq), sum(self.lk)
        self.max_q, self.max_k = max(self.lq), max(self.lk)
        self.pairs = visible_pairs(self.lq, self.lk)
        self.shape = dict(B=len(self.lq), H=H, total_q=self.tq, total_k=self.tk, max_seqlen_q=self.max_q, max_seqlen_k=self.max_k,
                          visible_pairs=self.pairs, flop=2 * self.pairs * H * (3 * D + 2 * D_V))
        self.copies = max(2, math.ceil(300e6 / (2 * self.tk * H * (D + D_V))))
        self.scale = D ** -0.5
        self.enum = convert_triton_dtype(torch.bfloat16)
        mk = lambda *s: (torch.randn(*s, device=dev) * 0.8).to(torch.bfloat16)  # noqa: E731
        self.Q, self.dO = mk(self.tq, H, D), mk(self.tq, H, D_V)
        self.K = [mk(self.tk, H, D) for _ in range(self.copies)]
        self.V = [mk(self.tk, H, D_V) for _ in range(self.copies)]
        cu = lambda ls: torch.tensor([0] + torch.tensor(ls).cumsum(0).tolist(), dtype=torch.int32, device=dev)  # noqa: E731
        self.cu_q, self.cu_k = cu(self.lq), cu(self.lk)
        # the forward's own O and L of every copy (the matrix forward; not timed)
        self.OL = [fa.flash_attention_mla_prefill_forward(self.Q, k, v, self.cu_q, self.cu_k, self.max_q, self.max_k, dev, causal=True,
                                                          scale=self.scale) for k, v in zip(self.K, self.V)]
        self.D = torch.empty(2, H, self.tq, dtype=torch.float32, device=dev)
        self.i = 0

    def _next(self):
        self.i = (self.i + 1) % self.copies
        return self.i

    def dv(self, variant):
        torch = self.torch
        dQ, dK, dV = torch.empty_like(self.Q), torch.empty_like(self.K[0]), torch.empty_like(self.V[0])

        def run():
            i = self._next()
            O, L = self.OL[i]
            self._lib.fa2_bwd_varlen_dv(self.Q, self.K[i], self.V[i], O, self.dO, L, dQ, dK, dV, self.D, self.cu_q, self.cu_k, self.max_q,
                                        self.max_k, self.enum, causal=True, scale=self.scale,
                                        variant=self._lib.BWD_VARLEN_DV_VARIANTS[variant])
        return run

    def padded(self):
        """the route without the entry point: V, O, dO zero-padded to 192 columns outside the timed calls"""
        pad = lambda t: self.torch.nn.functional.pad(t, (0, D - D_V))  # noqa: E731
        V, O, dO = [pad(v) for v in self.V], [pad(o) for o, _ in self.OL], pad(self.dO)

        def run():
            i = self._next()
            self.fa.flash_attention_varlen_backward(self.Q, self.K[i], V[i], O[i], dO, self.OL[i][1], self.cu_q, self.cu_k, self.max_q,
                                                    self.max_k, self.dev, causal=True, scale=self.scale)
        return run

    def d128(self):
        torch = self.torch
        Q, dO = self.Q[..., :128].contiguous(), self.dO
        K = [k[..., :128].contiguous() for k in self.K]
        OL = [self.fa.flash_attention_varlen_forward(Q, k, v, self.cu_q, self.cu_k, self.max_q, self.max_k, self.dev, causal=True,
                                                     scale=self.scale) for k, v in zip(K, self.V)]
        dQ, dK, dV = torch.empty_like(Q), torch.empty_like(K[0]), torch.empty_like(self.V[0])

        def run():
            i = self._next()
            self._lib.fa2_bwd_varlen(Q, K[i], self.V[i], OL[i][0], dO, OL[i][1], dQ, dK, dV, self.D, self.cu_q, self.cu_k, self.max_q,
                                     self.max_k, self.enum, causal=True, scale=self.scale)
        return run

    def sdpa(self):
        """-> (run, None) or (None, reason): forward and backward of one call per sequence"""
        torch = self.torch
        from torch.nn.attention import SDPBackend, sdpa_kernel
        F = torch.nn.functional
        sq, sk = self.cu_q.tolist(), self.cu_k.tolist()
        views = lambda t, s, b: t[s[b]:s[b + 1]].transpose(0, 1).unsqueeze(0)  # noqa: E731
        square = all(a == b for a, b in zip(self.lq, self.lk))
        masks = None if square else [torch.ones(nq, nk, dtype=torch.bool, device=self.dev).tril(nk - nq) for nq, nk in zip(self.lq, self.lk)]

        def run(backends):
            i = self._next()
            with sdpa_kernel(backends):
                for b in range(len(self.lq)):
                    q, k, v = (views(t, s, b).detach().requires_grad_() for t, s in ((self.Q, sq), (self.K[i], sk), (self.V[i], sk)))
                    if square:
                        o = F.scaled_dot_product_attention(q, k, v, is_causal=True, scale=self.scale)
                    else:
                        o = F.scaled_dot_product_attention(q, k, v, attn_mask=masks[b], scale=self.scale)
                    o.backward(views(self.dO, sq, b))

        fused = [SDPBackend.FLASH_ATTENTION, SDPBackend.EFFICIENT_ATTENTION]
        try:
            run(fused)
            torch.cuda.synchronize()
            return (lambda: run(fused)), None
        except RuntimeError as e:
            reason = "no fused backend: " + str(e).splitlines()[0][:120]
        score_bytes = 2 * self.H * max(nq * nk for nq, nk in zip(self.lq, self.lk))
        if score_bytes > 8 << 30:
            return None, reason + f"; the math backend's score matrix is {score_bytes >> 30} GiB"
        return (lambda: run([SDPBackend.MATH])), None


def slow_iters(shape, iters):
    """the VALU kernels run this shape's pairs at well under a TFLOP/s: fewer calls where one takes a large fraction of a second"""
    return max(2, min(iters, int(5e11 / shape["flop"])))


def run_pass(name, args):
    """The traced child: each side warmed, then run back to back; the kernel trace holds the times."""
    import torch
    c = Case(name, torch.device("cuda:0"))
    sdpa, reason = (None, "not asked for") if args.no_sdpa else c.sdpa()
    n_sdpa = min(args.iters, 5)
    if sdpa:
        try:
            for _ in range(2):
                sdpa()
            torch.cuda.synchronize()
        except RuntimeError as e:  # (out of memory in the math backend included)
            sdpa, reason = None, "sdpa failed: " + str(e).splitlines()[0][:120]
    slow = slow_iters(c.shape, args.iters)
    sides = [("auto", c.dv("auto"), 3, args.iters), ("mfma16dv", c.dv("mfma16dv"), 3, args.iters), ("generic", c.dv("generic"), 1, slow),
             ("padded", c.padded(), 1, slow), ("d128", c.d128(), 3, args.iters)]
    torch.cuda.synchronize()
    for _, f, warm, calls in sides:
        for _ in range(warm + calls):
            f()
        torch.cuda.synchronize()
    if sdpa:
        for _ in range(n_sdpa):
            sdpa()
        torch.cuda.synchronize()
    print(json.dumps(dict(case=name, sides=[(side, warm, calls) for side, _, warm, calls in sides], sdpa_calls=n_sdpa if sdpa else 0,
                          sdpa_skipped=reason if not sdpa else None, **c.shape)))


def child(out, name, args):
    os.makedirs(out, exist_ok=True)
    cmd = ["timeout", "-k", "10", str(args.child_timeout), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out,
           "--", sys.executable, os.path.abspath(__file__), "--iters", str(args.iters), "--pass-case", name] + (["--no-sdpa"] if args.no_sdpa else [])
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode != 0:  # a failed child ends the run: nothing more is started on the GPU
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
        sys.exit(p.returncode)
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def run_rocprof(names, args, fh):
    for name in names:
        out = os.path.join(args.rocprof, "prefill_bwd_" + name)
        info = child(out, name, args)
        rows = trace_rows(out)
        ours = [k for k, r in enumerate(rows) if any(n in r["Kernel_Name"] for n in OURS)]
        total = PER * sum(warm + calls for _, warm, calls in info["sides"])
        assert len(ours) == total, (len(ours), total)
        pos, sides = 0, {}
        for side, warm, calls in info.pop("sides"):
            seg = [rows[k] for k in ours[pos:pos + PER * (warm + calls)]]
            sides[side] = per_call(seg, PER, warm + calls, warm=warm)
            if side == "auto":
                us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3  # noqa: E731
                launches = {seg[j]["Kernel_Name"][:48]: round(sum(us(seg[PER * k + j]) for k in range(warm, warm + calls)) / calls, 2)
                            for j in range(PER)}
            pos += PER * (warm + calls)
        n = info.pop("sdpa_calls")
        sides["sdpa"] = None
        if n:
            rest = rows[ours[-1] + 1:]
            t = sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rest) / 1e3
            sides["sdpa"] = dict(avg_us=round(t / n, 2), calls=n, kernels=len(rest)) if rest else None
        a, m, g, y = sides["auto"], sides["mfma16dv"], sides["generic"], sides["d128"]
        emit(fh, kind="kernels", **info, auto_tflops=round(info["flop"] / a["avg_us"] / 1e6, 1),
             d128_tflops=round(info["flop"] / 1.30 / y["avg_us"] / 1e6, 1), mfma16dv_over_generic=round(m["avg_us"] / g["avg_us"], 4),
             ranges_overlap=m["max_us"] >= g["min_us"], auto_over_generic=round(a["avg_us"] / g["avg_us"], 4),
             auto_over_padded=round(a["avg_us"] / sides["padded"]["avg_us"], 4), auto_over_d128=round(a["avg_us"] / y["avg_us"], 4),
             auto_over_sdpa=round(a["avg_us"] / sides["sdpa"]["avg_us"], 4) if sides["sdpa"] else None, launches=launches, **sides)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rocprof", metavar="DIR", default=os.path.join(ROOT, "bench_out", "mla_traces"),
                    help="the traces of the rocprofv3 children go under DIR")
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--no-sdpa", action="store_true", help="leave the torch side out")
    ap.add_argument("--pass-case", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    if args.pass_case:
        return run_pass(args.pass_case, args)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fh:
        run_rocprof(args.cases.split(","), args, fh)


if __name__ == "__main__":
    main()
