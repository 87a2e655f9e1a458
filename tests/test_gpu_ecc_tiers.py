"""GPU tier (-m gpu): the loop bodies of k_rows_fast's eccentric form on a hand-built catalog (tests/ecc_tier_catalog.py).

The window plan gives every accepted window of the eccentric form one of three bodies (E1, E2, the general five-trip body);
a wave of the row kernel runs the loop compiled for its window's body.  azh_last_window_ecc_tiers reads the plan back, which
proves that every body ran; every row is held to the oracle at the gates of tests/test_gpu_parity.py and to the generic
kernels (fast path off) at the same gates; the error flags equal the oracle's; and both read-backs of the plan equal the
plan evaluated on the host (tests/host_emul/emul_ecc_tiers.cpp), which knows nothing of how the library was built:
azh_last_window_tiers reports what it reported before the eccentric form had tiers.
Shapes: 200 one-minute steps in segments of 128 (two windows per row, the second ending in a partial iteration of 8 lanes),
a day of 1,440 steps with the automatic segment length, and a (jd, fr) grid, whose bounds widen by the grid's deviations;
positions only and fp32 outputs on the 200-step shape.  The catalog is launched beside 200 near-circular members, so that the
eccentric launch takes the bulk's segment length.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ecc_tier_catalog  # noqa: E402
import ecc_tier_study as study  # noqa: E402

pytestmark = pytest.mark.gpu

TOL_R = 1e-6   # km    (tests/test_gpu_parity.py)
TOL_V = 1e-9   # km/s
F32_HALF_ULP = 2.0 ** -24  # fp32 rows of the eccentric form: fp64 arithmetic, one rounding to nearest of every component


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as g
    g.build()
    from astroz_amd import _native
    assert _native.device_count() >= 1, "no HIP device: GPU tests must run on the MI355X box"
    return _native


@pytest.fixture(scope="module")
def fleet(native, orc, tmp_path_factory):
    pairs = ecc_tier_catalog.ecc_pairs() + ecc_tier_catalog.filler_pairs()
    dev = native.DeviceConstellation.from_tle_lines(pairs, 1, 0)
    cat = orc.Catalog.from_pairs(pairs, 1)
    assert dev.n == len(pairs) and dev.n_sdp4 == 0
    return dev, cat, pairs, study.load(str(tmp_path_factory.mktemp("emul_ecc_tiers")))


def _run(native, dev, times, off, vel=True, f32=False):
    import torch
    n = len(times)
    dt = torch.float32 if f32 else torch.float64
    pos = torch.full((dev.n, n, 3), float("nan"), dtype=dt, device="cuda")
    v = torch.full((dev.n, n, 3), float("nan"), dtype=dt, device="cuda") if vel else None
    err = torch.empty((dev.n, n), dtype=torch.uint8, device="cuda")
    dev.propagate_device(times, off, pos.data_ptr(), v.data_ptr() if vel else None, layout=native.SAT_MAJOR, d_err=err.data_ptr(), f32=f32)
    dev.synchronize()
    return pos.cpu().numpy().astype(np.float64), (v.cpu().numpy().astype(np.float64) if vel else None), err.cpu().numpy()


def _check(native, orc, fleet, times, off, tile, quasi=False, other_outputs=False):
    dev, cat, pairs, E = fleet
    n = len(times)
    e0, p0, v0 = cat.propagate(times, off, layout=orc.SAT_MAJOR)
    pos, vel, err = _run(native, dev, times, off)
    path = dev.last_path()
    assert path & native.PATH_ROWS_FAST and bool(path & native.PATH_QUASI_UNIFORM) == quasi, path
    tiers, bodies = dev.last_window_tiers(), dev.last_window_ecc_tiers()
    print(tiers, bodies)
    # every body ran, and the new read-back splits the old one's eccentric count
    assert all(bodies[k] >= 5 for k in ("e1", "e2", "general")), bodies
    assert sum(bodies.values()) == tiers["ecc"] and tiers["rejected"] >= 2
    # both read-backs against the plan evaluated on the host
    step = (times[-1] - times[0]) / (n - 1)
    four, three = study.plan_counts(E, orc, pairs, times[0], step, n, off, tile, tile, study.DELTA_MAX if quasi else 0.0)
    assert tiers == four and bodies == three, (tiers, four, bodies, three)
    assert np.array_equal(err, e0)  # the error flags are clean
    assert not e0.any()
    dr, dv = float(np.abs(pos - p0).max()), float(np.abs(vel - v0).max())
    print("pos+vel: max|dr| = %.3e km, max|dv| = %.3e km/s" % (dr, dv))
    assert dr < TOL_R and dv < TOL_V, (dr, dv)
    # the generic kernels on the same grid
    dev.set_fast_path(False)
    try:
        pos2, vel2, _ = _run(native, dev, times, off)
        assert not dev.last_path() & native.PATH_ROWS_FAST
        assert not any(dev.last_window_ecc_tiers().values())
    finally:
        dev.set_fast_path(True)
    dr2, dv2 = float(np.abs(pos - pos2).max()), float(np.abs(vel - vel2).max())
    print("fast vs generic: max|dr| = %.3e km, max|dv| = %.3e km/s" % (dr2, dv2))
    assert dr2 < TOL_R and dv2 < TOL_V, (dr2, dv2)
    if other_outputs:
        # positions only and fp32 rows: the other instantiations of the eccentric kernel
        pos1, _, err1 = _run(native, dev, times, off, vel=False)
        assert dev.last_window_ecc_tiers() == bodies and np.array_equal(err1, e0)
        dr1 = float(np.abs(pos1 - p0).max())
        assert dr1 < TOL_R, dr1
        pos3, vel3, err3 = _run(native, dev, times, off, f32=True)
        assert all(v >= 5 for v in dev.last_window_ecc_tiers().values()) and np.array_equal(err3, e0)
        # (the eccentric rows: the near-circular ones take the packed fp32 kernel and its own, documented tolerance)
        ecc = np.array([r[3] >= 0.0025 for r in ecc_tier_catalog.ecc_rows()] + [False] * (dev.n - len(ecc_tier_catalog.ecc_rows())))
        dr3, dv3 = float(np.abs(pos3 - p0)[ecc].max()), float(np.abs(vel3 - v0)[ecc].max())
        print("positions only: max|dr| = %.3e km; fp32 rows of the eccentric form: max|dr| = %.3e km, max|dv| = %.3e km/s" % (dr1, dr3, dv3))
        assert (np.abs(pos3 - p0)[ecc] <= np.abs(p0[ecc]) * F32_HALF_ULP + TOL_R).all()
        assert (np.abs(vel3 - v0)[ecc] <= np.abs(v0[ecc]) * F32_HALF_ULP + TOL_V).all()


def test_two_windows_per_row_with_a_partial_iteration(native, orc, fleet):
    from astroz_amd import synth
    dev = fleet[0]
    dev.set_time_tile(128)
    try:
        _check(native, orc, fleet, np.arange(200, dtype=np.float64), (synth.START_JD - dev.epochs) * 1440.0, 128, other_outputs=True)
    finally:
        dev.set_time_tile(0)


def test_a_day_with_the_automatic_segments(native, orc, fleet):
    from astroz_amd import synth
    dev = fleet[0]
    _check(native, orc, fleet, np.arange(1440, dtype=np.float64), (synth.START_JD - dev.epochs) * 1440.0, 256)


def test_quasi_uniform_grid_widens_the_bounds(native, orc, fleet):
    dev = fleet[0]
    times, off = ecc_tier_catalog.jdfr_times(200, dev.epochs)
    dev.set_time_tile(128)
    try:
        _check(native, orc, fleet, times, off, 128, quasi=True)
    finally:
        dev.set_time_tile(0)
