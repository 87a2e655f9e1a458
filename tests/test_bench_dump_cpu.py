"""bench.py --dump-outputs (no GPU): the written arrays stay under the budget, are the same seeded satellite sample on
every call, hold exactly the values of the rows they name, and keep the output dtype."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _files(d):
    return {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_headline_shape_is_sampled_under_the_budget(tmp_path):
    g = torch.Generator().manual_seed(3)
    pos = torch.randn(13478, 1440, 3, dtype=torch.float64, generator=g)
    vel = torch.randn(13478, 1440, 3, dtype=torch.float64, generator=g)
    w = bench.dump_outputs(str(tmp_path / "a"), [("positions", pos), ("velocities", vel)], 0, 13478)
    bench.dump_outputs(str(tmp_path / "b"), [("positions", pos), ("velocities", vel)], 0, 13478)
    a, b = _files(tmp_path / "a"), _files(tmp_path / "b")
    assert sorted(a) == sorted(w) == ["positions.npy", "sat_index.npy", "velocities.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in a) <= bench.DUMP_BUDGET
    assert all(np.array_equal(a[f], b[f]) for f in a)
    rows = a["sat_index.npy"].astype(np.int64)
    assert a["sat_index.npy"].dtype == np.float64 and 100 < len(rows) < 13478
    assert np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < 13478
    assert np.array_equal(a["positions.npy"], pos.numpy()[rows]) and np.array_equal(a["velocities.npy"], vel.numpy()[rows])


def test_small_time_major_f32_output_is_written_whole(tmp_path):
    pos = torch.randn(200, 37, 3, dtype=torch.float32)
    bench.dump_outputs(str(tmp_path), [("positions", pos)], 1, 37)
    f = _files(tmp_path)
    assert f["positions.npy"].dtype == np.float32 and np.array_equal(f["positions.npy"], pos.numpy())
    assert np.array_equal(f["sat_index.npy"], np.arange(37.0))
