"""The host path of training attention against the recorded behaviour of the commit before its consolidation: every code and message
of the twenty launching entry points, the order of their checks, the kernel each valid call launches first and the static tile table
(tests/train_host_cases.py, tests/golden/train_host_calls.json).  The calls are made by a fresh child process that sees no device, so
a call that passes the checks fails at its first launch instead of running on a fake pointer; where a device stays visible the child
makes no call."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

import train_host_cases as cases


def test_recorded_calls_replay_without_a_mismatch():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "train_host_cases.py"), "--replay"], env=env, capture_output=True,
                         text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    result = json.loads(out.stdout.strip().splitlines()[-1])
    if "skipped" in result:
        pytest.skip(result["skipped"])
    assert result["mismatches"] == [], "\n".join(result["mismatches"][:40])


def test_fixture_covers_every_entry_point_and_kind():
    with open(cases.FIXTURE) as f:
        fixture = json.load(f)
    assert os.path.getsize(cases.FIXTURE) < 100 * 1024
    assert fixture["digest"] == cases.digest()
    assert len(cases.ENTRY_POINTS) == 20
    counts = cases.counts(fixture)
    for name in cases.ENTRY_POINTS:
        assert counts["singles"][name] == len(cases.singles(name)) >= 1, name
        assert counts["pairs"][name] == len(cases.pairs(name)) >= 1, name
        assert counts["valid"][name] >= 1, name
    assert counts["valid_stored"] == len(cases.valid())
    helpers = dict(cases.helpers())
    assert set(helpers) == {"fa2_query_tile_scaled", "fa2_query_tile", "fa2_query_tile_ex"}
    for name, grid in helpers.items():
        assert counts["helpers"][name] == len(grid) >= 1, name
    assert cases.picked(fixture) >= set(cases.PICKED)  # the grid reaches every `return` of pick_variant
