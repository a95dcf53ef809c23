#!/usr/bin/env python3
"""Un-absorbed MLA prefill (fa2_fwd_varlen_dv: d = 192, d_v = 128), bf16, causal, H_kv = H; JSON lines appended to
profiles/mla/bench_mla_prefill.jsonl.  The protocol is benchmarks/bench_mla_varlen.py's: kernel times come from a `rocprofv3
--kernel-trace --stats` child per shape (a fresh process, under its own `timeout -k 10`; the first non-zero status ends the run),
every side rotates over enough copies of K and V to exceed the 256 MiB last-level cache, each side is warmed (calls not counted) and
then run back to back, and avg, min-max and stddev are reported per call.

Shapes (H in {16, 128}):
  uniform   a uniform batch of 4 x 4096;
  long      one 32 Ki sequence;
  ragged    a seeded log-uniform mix of 16 lengths in [100, 8192];
  chunk     a chunk of 2048 queries over 16384 keys (bottom-right causal).

Sides of one child:
  auto      the call under AUTO (the matrix kernel mfma16dv);
  generic   the same call with the VALU form forced;
  padded    the only route without this entry point: fa2_fwd_varlen with V zero-padded to 192 columns (padded once, outside the timed
            calls; it lands on the VALU kernel fa2_generic), O 192 wide;
  d128      fa2_fwd_varlen at d = 128 on the same lengths (mfma16d_w4): the yardstick.  The FLOP ratio to it is (192 + 128) / (128 +
            128) = 1.25; auto_over_d128 is the time ratio;
  sdpa      torch.nn.functional.scaled_dot_product_attention, one call per sequence (fused backends first; the math backend only
            where its score matrix stays below 8 GiB; null with the reason where neither runs).
The kernel trace is cut into the library's sides by dispatch order (one fa2_fwd kernel per call); sdpa's timed calls are the rows
behind the last of them (its warm-up runs first).

TFLOP/s count 2 * visible pairs * H * (d + d_v)."""
import argparse
import json
import math
import os
import random
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_mla_decode import emit, per_call, trace_rows  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "mla", "bench_mla_prefill.jsonl")
D, D_V = 192, 128


def ragged_lengths(seed=0, count=16, lo=100, hi=8192):
    rng = random.Random(seed)
    return [int(math.exp(rng.uniform(math.log(lo), math.log(hi)))) for _ in range(count)]


# name -> (query lengths, key lengths)
BATCHES = {"uniform": ([4096] * 4, [4096] * 4), "long": ([32768], [32768]), "ragged": (ragged_lengths(), ragged_lengths()),
           "chunk": ([2048], [16384])}
CASES = {f"{name}_h{H}": (name, H) for name in BATCHES for H in (16, 128)}


def visible_pairs(lq, lk):
    """bottom-right causal: query i of a sequence sees keys j <= i + (n_k - n_q)"""
    return sum(sum(max(0, min(nk, i + nk - nq + 1)) for i in range(nq)) for nq, nk in zip(lq, lk))


class Case:
    def __init__(self, name, dev):
        import torch
        from flash_attention_dlrs_amd import _lib
        from flash_attention_dlrs_amd.flash_attention_torch import convert_triton_dtype
        self.torch, self._lib, self.dev = torch, _lib, dev
        batch, H = CASES[name]
        self.lq, self.lk = BATCHES[batch]
        self.H, self.tq, self.tk = H, sum(self.lq), sum(self.lk)
        self.max_q, self.max_k = max(self.lq), max(self.lk)
        self.pairs = visible_pairs(self.lq, self.lk)
        self.shape = dict(B=len(self.lq), H=H, total_q=self.tq, total_k=self.tk, max_seqlen_q=self.max_q, max_seqlen_k=self.max_k,
                          visible_pairs=self.pairs, flop=2 * self.pairs * H * (D + D_V))
        self.copies = max(2, math.ceil(300e6 / (2 * self.tk * H * (D + D_V))))
        self.scale = D ** -0.5
        self.enum = convert_triton_dtype(torch.bfloat16)
        mk = lambda *s: (torch.randn(*s, device=dev) * 0.8).to(torch.bfloat16)  # noqa: E731
        self.Q = mk(self.tq, H, D)
        self.K = [mk(self.tk, H, D) for _ in range(self.copies)]
        self.V = [mk(self.tk, H, D_V) for _ in range(self.copies)]
        cu = lambda ls: torch.tensor([0] + torch.tensor(ls).cumsum(0).tolist(), dtype=torch.int32, device=dev)  # noqa: E731
        self.cu_q, self.cu_k = cu(self.lq), cu(self.lk)
        self.L = torch.empty(H, self.tq, dtype=torch.bfloat16, device=dev)
        self.i = 0

    def _next(self):
        self.i = (self.i + 1) % self.copies
        return self.i

    def dv(self, variant):
        O = self.torch.empty(self.tq, self.H, D_V, dtype=self.torch.bfloat16, device=self.dev)

        def run():
            i = self._next()
            self._lib.fa2_fwd_varlen_dv(self.Q, self.K[i], self.V[i], O, self.L, self.cu_q, self.cu_k, self.max_q, self.max_k, self.enum,
                                        causal=True, scale=self.scale, variant=self._lib.VARLEN_DV_VARIANTS[variant])
        return run

    def varlen(self, d):
        """fa2_fwd_varlen under AUTO at head size d: 192 with V zero-padded (the route without the entry point), or the d = 128 yardstick"""
        torch = self.torch
        if d == D:
            Q, K = self.Q, self.K
            V = [torch.nn.functional.pad(v, (0, D - D_V)) for v in self.V]
        else:
            Q, K, V = self.Q[..., :d].contiguous(), [k[..., :d].contiguous() for k in self.K], self.V
        O = torch.empty(self.tq, self.H, d, dtype=torch.bfloat16, device=self.dev)

        def run():
            i = self._next()
            self._lib.fa2_fwd_varlen(Q, K[i], V[i], O, self.L, self.cu_q, self.cu_k, self.max_q, self.max_k, self.enum, causal=True,
                                     scale=self.scale)
        return run

    def sdpa(self):
        """-> (run, None) or (None, reason)"""
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
                    q, k, v = views(self.Q, sq, b), views(self.K[i], sk, b), views(self.V[i], sk, b)
                    if square:
                        F.scaled_dot_product_attention(q, k, v, is_causal=True, scale=self.scale)
                    else:
                        F.scaled_dot_product_attention(q, k, v, attn_mask=masks[b], scale=self.scale)

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
    """the VALU kernels run this shape's pairs at a few TFLOP/s: fewer calls where one takes a large fraction of a second"""
    return max(2, min(iters, int(2e12 / shape["flop"])))


def run_pass(name, args):
    """The traced child: each side warmed, then run back to back; the kernel trace holds the times."""
    import torch
    c = Case(name, torch.device("cuda:0"))
    sdpa, reason = c.sdpa()
    n_sdpa = min(args.iters, 5)
    if sdpa:
        try:
            for _ in range(2):
                sdpa()
            torch.cuda.synchronize()
        except RuntimeError as e:  # (out of memory in the math backend included)
            sdpa, reason = None, "sdpa failed: " + str(e).splitlines()[0][:120]
    slow =slow_iters(c.shape, args.iters)
    sides = [("auto", c.dv("auto"), 3, args.iters), ("generic", c.dv("generic"), 1, slow), ("padded", c.varlen(D), 1, slow),
             ("d128", c.varlen(128), 3, args.iters)]
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
           "--", sys.executable, os.path.abspath(__file__), "--iters", str(args.iters), "--pass-case", name]
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode != 0:  # a failed child ends the run: nothing more is started on the GPU
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
        sys.exit(p.returncode)
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def run_rocprof(names, args, fh):
    for name in names:
        out = os.path.join(args.rocprof, "prefill_" + name)
        info = child(out, name, args)
        rows = trace_rows(out)
        ours = [k for k, r in enumerate(rows) if "fa2_fwd" in r["Kernel_Name"]]
        pos, sides = 0, {}
        for side, warm, calls in info.pop("sides"):
            seg = [rows[k] for k in ours[pos:pos + warm + calls]]
            sides[side] = per_call(seg, 1, warm + calls, warm=warm)
            pos += warm + calls
        assert pos == len(ours), (pos, len(ours))
        n = info.pop("sdpa_calls")
        if n:
            rest = rows[ours[-1] + 1:]
            if rest and len(rest) % n == 0:
                sides["sdpa"] = per_call(rest, len(rest) // n, n, warm=0)
            else:  # (calls of unequal kernel counts cannot be cut apart: the average alone)
                total = sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rest) / 1e3
                sides["sdpa"] = dict(avg_us=round(total / n, 2), calls=n, kernels=len(rest)) if rest else None
        else:
            sides["sdpa"] = None
        a, g, y = sides["auto"], sides["generic"], sides["d128"]
        emit(fh, kind="kernels", **info, auto_tflops=round(info["flop"] / a["avg_us"] / 1e6, 1),
             d128_tflops=round(info["flop"] / 1.25 / y["avg_us"] / 1e6, 1), auto_over_generic=round(a["avg_us"] / g["avg_us"], 4),
             ranges_overlap=a["max_us"] >= g["min_us"], auto_over_padded=round(a["avg_us"] / sides["padded"]["avg_us"], 4),
             auto_over_d128=round(a["avg_us"] / y["avg_us"], 4),
             auto_over_sdpa=round(a["avg_us"] / sides["sdpa"]["avg_us"], 4) if sides["sdpa"] else None, **sides)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rocprof", metavar="DIR", default=os.path.join(ROOT, "bench_out", "mla_traces"),
                    help="the traces of the rocprofv3 children go under DIR")
    ap.add_argument("--child-timeout", type=int, default=240)
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
