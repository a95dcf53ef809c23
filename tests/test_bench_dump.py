"""bench.py --dump-outputs DIR: what the last timed step returned, written as float32 .npy files -- whole when small, a fixed
seeded sample of the flattened values when large -- so that two builds can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

import bench


def test_dump_writes_small_arrays_whole_and_large_ones_as_a_fixed_sample(tmp_path):
    g = torch.Generator().manual_seed(3)
    small = torch.randn(2, 3, 5, 1, generator=g).to(torch.bfloat16)
    large = torch.randn(4, 8, 64, 16, generator=g).to(torch.float16)     # 32768 elements > max_elems below
    info = bench.dump_outputs(str(tmp_path / "a"), {"L": small, "O": large, "none": None}, max_elems=1000)
    assert sorted(os.listdir(tmp_path / "a")) == ["L.npy", "O.npy"]
    L, O = np.load(tmp_path / "a" / "L.npy"), np.load(tmp_path / "a" / "O.npy")
    assert L.dtype == np.float32 and O.dtype == np.float32
    assert L.shape == (2, 3, 5, 1) and np.array_equal(L, small.float().numpy()) and info["L"] == ((2, 3, 5, 1), True)
    assert O.ndim == 1 and 900 < O.size <= 1000 and info["O"] == (O.shape, False)
    flat = large.float().numpy().reshape(-1)
    assert np.isin(O, flat).all()
    # the same shape gives the same positions in every run: a second dump of the same tensor is identical
    bench.dump_outputs(str(tmp_path / "b"), {"O": large}, max_elems=1000)
    assert np.array_equal(np.load(tmp_path / "b" / "O.npy"), O)


def test_dump_budget_keeps_the_flagship_outputs_under_64_mb():
    c = bench.CONFIGS["c3"]
    n_O, n_L = c["B"] * c["H"] * c["N"] * c["d"], c["B"] * c["H"] * c["N"]
    assert 4 * (min(n_O, bench.DUMP_MAX_ELEMS) + min(n_L, bench.DUMP_MAX_ELEMS)) <= 64 * 10 ** 6


@pytest.mark.gpu
def test_bench_dumps_what_the_timed_path_computed(tmp_path):
    """c2 (B2 H8 N1024 d64 fp16) is small enough to be written whole: the dump equals a direct call on the same seeded inputs."""
    out = subprocess.run([sys.executable, "bench.py", "--config", "c2", "--steps", "4", "--warmup", "1", "--no-cpu-baseline",
                          "--no-extras", "--dump-outputs", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    j = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0])
    assert j["steps"] == 4 and j["ms_per_step"] > 0
    O, L = np.load(tmp_path / "O.npy"), np.load(tmp_path / "L.npy")
    assert O.dtype == np.float32 and O.shape == (2, 8, 1024, 64) and L.shape == (2, 8, 1024, 1)

    from flash_attention_dlrs_amd import flash_attention_forward
    c, dev = bench.CONFIGS["c2"], torch.device("cuda:0")
    torch.manual_seed(42)
    Q, K, V = (torch.randn(c["B"], c["H"], c["N"], c["d"], device=dev).to(torch.float16) for _ in range(3))
    O_ref, L_ref = flash_attention_forward(Q, K, V, dev, causal=c["causal"])
    torch.cuda.synchronize()
    assert np.array_equal(O, O_ref.float().cpu().numpy())
    assert np.array_equal(L, L_ref.float().cpu().numpy())
