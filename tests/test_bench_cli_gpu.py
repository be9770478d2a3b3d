"""bench.py as a command: a plain run prints the headline line and nothing that takes runs of its own, --dump-outputs
writes the last timed step's results (equal from run to run, and equal to the oracle's replay of the same seeded
batches), --full adds the figures a plain run leaves out. Small sizes: 20k flowIds, 1.2M requests per step (more
than the dump keeps, so the row sample is exercised), 3 timed steps after 1 warm-up step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle.binding import ClusterTokenService
from sentinel_amd import abi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_FLOWS, N_REQ, STEPS, WARMUP = 20_000, 1_200_000, 3, 1
SIZES = ["--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP), "--flows", str(N_FLOWS),
         "--requests", str(N_REQ)]
FIELDS = ("status", "remaining", "wait_ms")


def _bench(*extra):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SIZES + list(extra), capture_output=True,
                         text=True, timeout=120, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def _load(d):
    return {n[:-4]: np.load(os.path.join(d, n)) for n in sorted(os.listdir(d))}


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("dump") / "out")
    return _bench("--dump-outputs", d), d


def test_plain_run_prints_the_headline_only(plain):
    res, _ = plain
    assert res["steps"] == STEPS and res["warmup"] == WARMUP
    assert res["unit"] == "decisions/s" and res["higher_is_better"] is True and res["dtype"] == "int64"
    assert res["ms_per_step"] > 0
    assert res["value"] == pytest.approx(N_REQ / (res["ms_per_step"] / 1000.0), rel=1e-9)
    assert not {"phases_ms", "end_to_end", "cpu_baseline"} & set(res)


def test_dump_is_the_last_timed_step_of_the_seeded_trace(plain):
    from bench import ShardWorkload
    _, d = plain
    got = _load(d)
    assert set(got) == set(FIELDS) | {"sample_index"}
    assert all(a.dtype == np.float64 for a in got.values())
    assert sum(os.path.getsize(os.path.join(d, n)) for n in os.listdir(d)) <= 64 << 20
    idx = got["sample_index"].astype(np.int64)
    assert len(idx) == 1_000_000 and np.all(np.diff(idx) > 0) and 0 <= idx[0] and idx[-1] < N_REQ
    wl = ShardWorkload(N_FLOWS, N_REQ, 0, 1, torch.device("cuda:0"))
    ns = np.zeros(1, abi.NS_DTYPE)
    ns["connected_count"] = 1
    ns["max_allowed_qps"] = 30000
    ora = ClusterTokenService()
    ora.set_namespaces(ns)
    ora.load_rules(wl.rules)
    for b in range(WARMUP + STEPS):
        want = ora.decide(wl.batch(b).cpu().numpy().view(abi.REQ_DTYPE))
    for f in FIELDS:
        assert np.array_equal(got[f], want[f][idx].astype(np.float64)), f
    assert len(np.unique(got["status"])) > 1


def test_dump_is_the_same_from_run_to_run(plain, tmp_path):
    _, d = plain
    d2 = str(tmp_path / "again")
    _bench("--dump-outputs", d2)
    first, second = _load(d), _load(d2)
    assert set(first) == set(second)
    for name in first:
        assert np.array_equal(first[name], second[name]), name


def test_full_adds_what_the_plain_run_leaves_out():
    res = _bench("--full", "--no-cpu-baseline", "--e2e-batches", "2")
    assert res["steps"] == STEPS and res["ms_per_step"] > 0
    assert {"sort", "walk", "device_total_one_batch_unpipelined", "long_segments"} <= set(res["phases_ms"])
    assert res["end_to_end"]["batches"] == 2 and res["end_to_end"]["value"] > 0
    assert "cpu_baseline" not in res
