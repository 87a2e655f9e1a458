"""GPU tier (-m gpu): the tiered loop bodies of k_rows_fast on a hand-built catalog (tests/tier_catalog.py).

The window plan gives every (satellite, time segment) window a body tier; a wave of the row kernel branches once into the
loop compiled for its tier.  azh_last_window_tiers reads the plan back, which proves that every body ran; every row is held
to the oracle at the gates of tests/test_gpu_parity.py and to the generic kernels (fast path off) at the same gates.
Shapes: 200 one-minute steps in segments of 128 (two windows per row, the second ending in a partial iteration of 8 lanes),
a day of 1,440 steps with the automatic segment length, and a (jd, fr) grid, whose bounds widen by the grid's deviations.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tier_catalog  # noqa: E402

pytestmark = pytest.mark.gpu

TOL_R = 1e-6   # km    (tests/test_gpu_parity.py)
TOL_V = 1e-9   # km/s


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as g
    g.build()
    from astroz_amd import _native
    assert _native.device_count() >= 1, "no HIP device: GPU tests must run on the MI355X box"
    return _native


@pytest.fixture(scope="module")
def fleet(native, orc):
    pairs = tier_catalog.tier_pairs()
    dev = native.DeviceConstellation.from_tle_lines(pairs, 1, 0)
    cat = orc.Catalog.from_pairs(pairs, 1)
    assert 35 <= dev.n <= 60 and dev.n_sdp4 == 0
    return dev, cat


def _run(native, dev, times, off, vel=True):
    import torch
    n = len(times)
    pos = torch.full((dev.n, n, 3), float("nan"), dtype=torch.float64, device="cuda")
    v = torch.full((dev.n, n, 3), float("nan"), dtype=torch.float64, device="cuda") if vel else None
    err = torch.empty((dev.n, n), dtype=torch.uint8, device="cuda")
    dev.propagate_device(times, off, pos.data_ptr(), v.data_ptr() if vel else None, layout=native.SAT_MAJOR, d_err=err.data_ptr())
    dev.synchronize()
    return pos.cpu().numpy(), (v.cpu().numpy() if vel else None), err.cpu().numpy()


def _check(native, orc, dev, cat, times, off, quasi=False):
    e0, p0, v0 = cat.propagate(times, off, layout=orc.SAT_MAJOR)
    assert not e0.any()
    pos, vel, err = _run(native, dev, times, off)
    path = dev.last_path()
    assert path & native.PATH_ROWS_FAST and bool(path & native.PATH_QUASI_UNIFORM) == quasi, path
    tiers = dev.last_window_tiers()
    print(tiers)
    assert all(tiers[k] > 0 for k in ("general", "eps", "ecc", "rejected")), tiers
    assert np.array_equal(err, e0)
    dr, dv = float(np.abs(pos - p0).max()), float(np.abs(vel - v0).max())
    print("pos+vel: max|dr| = %.3e km, max|dv| = %.3e km/s" % (dr, dv))
    assert dr < TOL_R and dv < TOL_V, (dr, dv)
    # positions only: its own instantiation of the kernel
    pos1, _, _ = _run(native, dev, times, off, vel=False)
    assert dev.last_window_tiers() == tiers
    dr1 = float(np.abs(pos1 - p0).max())
    assert dr1 < TOL_R, dr1
    # the generic kernels on the same grid
    dev.set_fast_path(False)
    try:
        pos2, vel2, _ = _run(native, dev, times, off)
        assert not dev.last_path() & native.PATH_ROWS_FAST
        assert not any(dev.last_window_tiers().values())
    finally:
        dev.set_fast_path(True)
    dr2, dv2 = float(np.abs(pos - pos2).max()), float(np.abs(vel - vel2).max())
    print("fast vs generic: max|dr| = %.3e km, max|dv| = %.3e km/s" % (dr2, dv2))
    assert dr2 < TOL_R and dv2 < TOL_V, (dr2, dv2)
    return tiers


def test_two_windows_per_row_with_a_partial_iteration(native, orc, fleet):
    from astroz_amd import synth
    dev, cat = fleet
    dev.set_time_tile(128)
    try:
        tiers = _check(native, orc, dev, cat, np.arange(200, dtype=np.float64), (synth.START_JD - dev.epochs) * 1440.0)
        # two windows per near-circular row (the eccentric form keeps its own segment length)
        n_ecc = sum(1 for _, l2 in tier_catalog.tier_pairs() if float("0." + l2[26:33]) >= 0.0025)
        near = tiers["general"] + tiers["eps"]
        assert 2 * (dev.n - n_ecc) - tiers["rejected"] <= near <= 2 * (dev.n - n_ecc), tiers
    finally:
        dev.set_time_tile(0)


def test_a_day_with_the_automatic_segments(native, orc, fleet):
    from astroz_amd import synth
    dev, cat = fleet
    _check(native, orc, dev, cat, np.arange(1440, dtype=np.float64), (synth.START_JD - dev.epochs) * 1440.0)


def test_quasi_uniform_grid_widens_the_tier_bounds(native, orc, fleet):
    dev, cat = fleet
    times, off = tier_catalog.jdfr_times(200, dev.epochs)
    dev.set_time_tile(128)
    try:
        _check(native, orc, dev, cat, times, off, quasi=True)
    finally:
        dev.set_time_tile(0)
