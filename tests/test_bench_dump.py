"""bench.dump_outputs (the writer behind bench.py --dump-outputs) on the host: one float64 array per field, every row
of a small output, a fixed ascending sample of a large one, the same indices on every call."""
import os
import sys

import numpy as np

from sentinel_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _records(n):
    r = np.zeros(n, abi.RES_DTYPE)
    r["status"] = np.arange(n) % 3
    r["remaining"] = np.arange(n, dtype=np.int64) * 7919 % 2147483647
    r["wait_ms"] = -np.arange(n) % 1000
    return r


def _load(d):
    return {n[:-4]: np.load(os.path.join(d, n)) for n in os.listdir(d)}


def test_small_output_is_written_whole(tmp_path):
    from bench import dump_outputs
    r = _records(1001)
    dump_outputs(str(tmp_path / "d"), r, suffix=".rank1")
    got = _load(str(tmp_path / "d"))
    assert set(got) == {"status.rank1", "remaining.rank1", "wait_ms.rank1", "sample_index.rank1"}
    assert np.array_equal(got["sample_index.rank1"], np.arange(1001))
    for f in r.dtype.names:
        assert got[f + ".rank1"].dtype == np.float64 and np.array_equal(got[f + ".rank1"], r[f])


def test_large_output_is_sampled_at_fixed_indices(tmp_path):
    from bench import dump_outputs
    r = _records(5000)
    dump_outputs(str(tmp_path / "a"), r, max_rows=777)
    dump_outputs(str(tmp_path / "b"), r, prefix="metric_", max_rows=777)
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    idx = a["sample_index"].astype(np.int64)
    assert len(idx) == 777 and np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < 5000
    assert np.array_equal(a["sample_index"], b["metric_sample_index"])
    for f in r.dtype.names:
        assert np.array_equal(a[f], r[f][idx]) and np.array_equal(b["metric_" + f], a[f])
