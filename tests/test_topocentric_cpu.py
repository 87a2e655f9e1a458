"""Topocentric look angles on the host (no GPU): azh_coords_topocentric -- the host twin of the kernels' AZ_OUT_TOPOCENTRIC
epilogue -- against geometric known answers, an independent numpy implementation and finite differences of two-body
trajectories; null-pointer checks of the new entry points."""
import numpy as np
import pytest

OMEGA = 7.292115146706979e-5  # rad/s
F = 1.0 / 298.257223563
E2 = 2.0 * F - F * F
A = 6378.137


def geodetic_to_ecef(lat_deg, lon_deg, alt_km):
    lat, lon = np.radians(lat_deg), np.radians(lon_deg)
    n = A / np.sqrt(1.0 - E2 * np.sin(lat) ** 2)
    return np.array([(n + alt_km) * np.cos(lat) * np.cos(lon), (n + alt_km) * np.cos(lat) * np.sin(lon),
                     (n * (1.0 - E2) + alt_km) * np.sin(lat)])


def enu_basis(lat_deg, lon_deg):
    lat, lon = np.radians(lat_deg), np.radians(lon_deg)
    e = np.array([-np.sin(lon), np.cos(lon), 0.0])
    n = np.array([-np.sin(lat) * np.cos(lon), -np.sin(lat) * np.sin(lon), np.cos(lat)])
    u = np.array([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)])
    return e, n, u


def rot(g):
    """TEME -> ECEF rotation about z by the Greenwich angle g."""
    c, s = np.cos(g), np.sin(g)
    return np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]])


def ecef_to_teme(x, g):
    return rot(g).T @ x


def numpy_topocentric(r_teme, v_teme, gmst, obs):
    """Independent implementation: rotation matrices, ENU basis vectors, hypot / arctan2."""
    R = rot(gmst)
    r = R @ r_teme
    rho = r - geodetic_to_ecef(*obs)
    e, n, u = enu_basis(obs[0], obs[1])
    E, N, U = rho @ e, rho @ n, rho @ u
    h = np.hypot(E, N)
    rng = np.sqrt(E * E + N * N + U * U)
    az = np.mod(np.arctan2(E, N), 2.0 * np.pi)
    el = np.arctan2(U, h)
    rhod = R @ v_teme - np.cross([0.0, 0.0, OMEGA], r)
    Ed, Nd, Ud = rhod @ e, rhod @ n, rhod @ u
    azd = (Ed * N - E * Nd) / (h * h)
    eld = (Ud * h - U * (E * Ed + N * Nd) / h) / (rng * rng)
    rngd = (E * Ed + N * Nd + U * Ud) / rng
    return np.array([az, el, rng]), np.array([azd, eld, rngd]), h


@pytest.fixture(scope="module")
def topo(native):
    L = native.lib()

    def f(r, v, gmst, obs, rates=True):
        r = np.ascontiguousarray(r, dtype=np.float64)
        v = None if v is None else np.ascontiguousarray(v, dtype=np.float64)
        o = np.ascontiguousarray(obs, dtype=np.float64)
        aer = np.full(3, np.nan)
        rate = np.full(3, np.nan)
        L.azh_coords_topocentric(r.ctypes.data, None if v is None else v.ctypes.data, float(gmst), o.ctypes.data,
                                 aer.ctypes.data, rate.ctypes.data if rates else None)
        return aer, rate
    return f


OBSERVERS = [(0.0, 0.0, 0.0), (47.3, 8.5, 0.4), (-33.9, 151.2, 0.05), (89.99, -45.0, 2.0), (90.0, 0.0, 0.0), (-90.0, 30.0, 1.0),
             (12.0, 180.0, 0.0), (-61.0, -180.0, 3.0), (35.0, -179.999, 0.1)]


@pytest.mark.parametrize("obs", OBSERVERS)
def test_known_answers(topo, obs):
    g = 1.234
    r_obs = geodetic_to_ecef(*obs)
    e, n, u = enu_basis(obs[0], obs[1])
    # on the observer's ellipsoid normal: straight up, range = altitude difference
    for alt in (400.0, 20000.0):
        aer, rate = topo(ecef_to_teme(geodetic_to_ecef(obs[0], obs[1], obs[2] + alt), g), np.zeros(3), g, obs)
        assert abs(aer[1] - np.pi / 2) <= 1e-12
        assert abs(aer[2] - alt) <= 1e-9
        assert aer[0] == 0.0 and rate[0] == 0.0  # exactly overhead: azimuth and its rate are 0
    # due N / E / S / W on the local horizon
    for vec, want in ((n, 0.0), (e, np.pi / 2), (-n, np.pi), (-e, 1.5 * np.pi)):
        aer, _ = topo(ecef_to_teme(r_obs + 1000.0 * vec, g), None, g, obs)
        assert abs(aer[1]) <= 1e-12
        dz = (aer[0] - want + np.pi) % (2 * np.pi) - np.pi
        assert abs(dz) <= 1e-12, (aer[0], want)
        assert 0.0 <= aer[0] < 2 * np.pi
        assert abs(aer[2] - 1000.0) <= 1e-9


def test_azimuth_range_and_null_velocity(topo):
    rng = np.random.default_rng(5)
    for _ in range(2000):
        obs = (rng.uniform(-90, 90), rng.uniform(-180, 180), rng.uniform(-0.4, 5))
        r = rng.normal(size=3)
        r *= rng.uniform(6500, 45000) / np.linalg.norm(r)
        aer, rate = topo(r, None, rng.uniform(0, 2 * np.pi), obs)
        assert 0.0 <= aer[0] < 2 * np.pi
        assert -np.pi / 2 <= aer[1] <= np.pi / 2
        assert (rate == 0.0).all()  # v = NULL -> rates 0


def test_matches_numpy_implementation(topo):
    rng = np.random.default_rng(7)
    worst = np.zeros(6)
    for _ in range(10_000):
        obs = (rng.uniform(-90, 90), rng.uniform(-180, 180), rng.uniform(-0.4, 5))
        r = rng.normal(size=3)
        r *= rng.uniform(6600, 45000) / np.linalg.norm(r)
        v = rng.normal(size=3) * 4.0
        g = rng.uniform(0, 2 * np.pi)
        aer, rate = topo(r, v, g, obs)
        a0, r0, h = numpy_topocentric(r, v, g, obs)
        if h < 10.0:
            continue
        daz = (aer[0] - a0[0] + np.pi) % (2 * np.pi) - np.pi
        worst = np.maximum(worst, [abs(daz), abs(aer[1] - a0[1]), abs(aer[2] - a0[2]) / a0[2],
                                   abs(rate[0] - r0[0]), abs(rate[1] - r0[1]), abs(rate[2] - r0[2])])
    # angles to 1e-12 rad, range to 1e-12 relative, rates to 1e-12 (rad/s, km/s)
    assert (worst <= 1e-12).all(), worst


def _kepler_track(a, e, inc, raan, argp, m0, t):
    """Exact two-body state (km, km/s) at t seconds."""
    mu = 398600.4418
    n = np.sqrt(mu / a ** 3)
    M = m0 + n * t
    E = M
    for _ in range(50):
        E = E - (E - e * np.sin(E) - M) / (1 - e * np.cos(E))
    cE, sE = np.cos(E), np.sin(E)
    b = a * np.sqrt(1 - e * e)
    x, y = a * (cE - e), b * sE
    Ed = n / (1 - e * cE)
    vx, vy = -a * sE * Ed, b * cE * Ed
    co, so, ci, si, cw, sw = np.cos(raan), np.sin(raan), np.cos(inc), np.sin(inc), np.cos(argp), np.sin(argp)
    P = np.array([co * cw - so * sw * ci, so * cw + co * sw * ci, sw * si])
    Q = np.array([-co * sw - so * cw * ci, -so * sw + co * cw * ci, cw * si])
    return x * P + y * Q, vx * P + vy * Q


def test_rates_match_finite_differences(topo):
    rng = np.random.default_rng(11)
    hstep = 1e-3  # s
    checked = 0
    for k in range(300):
        a = rng.choice([6778.0, 7200.0, 26560.0, 42164.0]) * rng.uniform(0.99, 1.01)
        e = rng.choice([0.0, 0.001, 0.05, 0.6]) if a < 30000 else rng.uniform(0.0, 0.3)
        a = max(a, 6700.0 / (1 - e))
        # (the mean anomaly and the Greenwich angle stay small at the evaluation point, t = 0: the rounding of an angle of
        # several radians, times 42,000 km, over 2 ms would be 1e-8 km/s of noise in the difference itself; argument of
        # perigee, node and observer longitude are random, so the geometry is not)
        el = (a, e, rng.uniform(0, np.pi), rng.uniform(0, 2 * np.pi), rng.uniform(0, 2 * np.pi), rng.uniform(-0.5, 0.5))
        obs = (rng.uniform(-89, 89), rng.uniform(-180, 180), rng.uniform(0, 3))
        g0 = rng.uniform(-0.5, 0.5)
        t = 0.0

        def at(ts):
            r, v = _kepler_track(*el, ts)
            return topo(r, v, g0 + OMEGA * ts, obs)

        aer, rate = at(t)
        ap, _ = at(t + hstep)
        am, _ = at(t - hstep)
        d = (ap - am) / (2 * hstep)
        d[0] = ((ap[0] - am[0] + np.pi) % (2 * np.pi) - np.pi) / (2 * hstep)
        assert abs(rate[2] - d[2]) <= 1e-8, (k, rate[2], d[2])
        hz = aer[2] * np.cos(aer[1])  # horizontal distance
        if hz >= 10.0:
            assert abs(rate[0] - d[0]) <= 1e-9, (k, rate[0], d[0])
            assert abs(rate[1] - d[1]) <= 1e-9, (k, rate[1], d[1])
            checked += 1
    assert checked > 250


def test_null_pointers(native):
    L = native.lib()
    t = np.arange(10.0)
    out = np.zeros(4, dtype=native.PASS_DTYPE)
    n = np.zeros(1, dtype=np.uint32)
    assert L.azh_set_observer(None, 10.0, 20.0, 0.0) == -101
    assert L.azh_find_passes_host(None, t.ctypes.data, len(t), None, 0.0, 10.0, out.ctypes.data, 4, n.ctypes.data) == -101
    assert L.azh_find_passes_device(None, t.ctypes.data, len(t), None, 0.0, 10.0, None, 4, None, None) == -101
    # the host twin ignores null inputs / outputs instead of crashing
    r, lla, aer = np.array([7000.0, 0, 0]), np.zeros(3), np.zeros(3)
    L.azh_coords_topocentric(None, None, 0.0, lla.ctypes.data, aer.ctypes.data, None)
    L.azh_coords_topocentric(r.ctypes.data, None, 0.0, None, aer.ctypes.data, None)
    L.azh_coords_topocentric(r.ctypes.data, None, 0.0, lla.ctypes.data, None, None)


def test_abi_constants(native):
    assert native.OUT_TOPOCENTRIC == 3 and native.OUTPUT_MODES["topocentric"] == 3
    assert native.PASS_DTYPE.itemsize == 64
    assert [native.PASS_DTYPE.fields[k][1] for k in ("flags", "grid_rise", "grid_culm", "grid_set")] == [48, 52, 56, 60]
    hdr = open(native.os.path.join(native._HERE, "..", "include", "astroz_hip.h")).read()
    assert "AZ_OUT_TOPOCENTRIC = 3" in hdr
    assert "#define AZH_PASS_UP_AT_START 1u" in hdr and "#define AZH_PASS_CUT_BY_ERROR 4u" in hdr


def test_python_argument_checks(native):
    import astroz_amd
    assert "passes" in astroz_amd.__all__
    with pytest.raises(ValueError):
        astroz_amd._check_output("topocentric", None)
    with pytest.raises(ValueError):
        astroz_amd._check_output("ecef", (1.0, 2.0, 0.0))
    with pytest.raises(ValueError):
        astroz_amd._check_output("horizon", None)
    astroz_amd._check_output("topocentric", (1.0, 2.0, 0.0))
    for bad in ((91.0, 0.0, 0.0), (np.nan, 0.0, 0.0), (0.0, np.inf, 0.0), (1.0, 2.0)):
        with pytest.raises(ValueError):
            astroz_amd.passes("unused", [0.0, 1.0], bad)
