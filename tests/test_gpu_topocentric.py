"""AZ_OUT_TOPOCENTRIC and the pass finder on the GPU: look angles against the oracle's ECEF output converted here, the device
epilogue against its host twin, observer changes under cached launches and graphs, passes against an independent scan."""
from datetime import datetime, timezone

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OMEGA = 7.292115146706979e-5
F = 1.0 / 298.257223563
E2 = 2.0 * F - F * F
A = 6378.137
OBS = (47.3, 8.5, 0.4)


def obs_frame(obs):
    lat, lon = np.radians(obs[0]), np.radians(obs[1])
    n = A / np.sqrt(1.0 - E2 * np.sin(lat) ** 2)
    r = np.array([(n + obs[2]) * np.cos(lat) * np.cos(lon), (n + obs[2]) * np.cos(lat) * np.sin(lon),
                  (n * (1.0 - E2) + obs[2]) * np.sin(lat)])
    e = np.array([-np.sin(lon), np.cos(lon), 0.0])
    nn = np.array([-np.sin(lat) * np.cos(lon), -np.sin(lat) * np.sin(lon), np.cos(lat)])
    u = np.array([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)])
    return r, np.stack([e, nn, u])


def topo_from_ecef(p, v, obs):
    """(..., 3) ECEF position / rotated velocity (the oracle's ECEF mode) -> (aer, aer rates, horizontal distance)."""
    r0, B = obs_frame(obs)
    enu = (p - r0) @ B.T
    E, N, U = enu[..., 0], enu[..., 1], enu[..., 2]
    h = np.hypot(E, N)
    rng = np.sqrt(h * h + U * U)
    aer = np.stack([np.mod(np.arctan2(E, N), 2 * np.pi), np.arctan2(U, h), rng], axis=-1)
    if v is None:
        return aer, None, h
    rd = v + OMEGA * np.stack([p[..., 1], -p[..., 0], np.zeros_like(p[..., 0])], axis=-1)  # - omega x r
    d = rd @ B.T
    Ed, Nd, Ud = d[..., 0], d[..., 1], d[..., 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        rate = np.stack([(Ed * N - E * Nd) / (h * h), (Ud * h * h - U * (E * Ed + N * Nd)) / (h * rng * rng),
                         (E * Ed + N * Nd + U * Ud) / rng], axis=-1)
    return aer, rate, h


def gate(aer, rate, ref_aer, ref_rate, h, ok, pos_tol=1e-6, rr_tol=1e-9, ar_tol=2e-9, az_rate_h=100.0, az_h=0.0):
    """Angles gated as displacements: range, |d el| * range, |d az| * h; rates: range rate, and |d el rate| * h, |d az rate| * h
    where h >= az_rate_h."""
    a, r0 = aer[ok], ref_aer[ok]
    hh = h[ok]
    daz = np.abs((a[:, 0] - r0[:, 0] + np.pi) % (2 * np.pi) - np.pi)
    d_rng, d_el, d_az = np.abs(a[:, 2] - r0[:, 2]), np.abs(a[:, 1] - r0[:, 1]) * r0[:, 2], daz * hh
    assert d_rng.max() <= pos_tol
    assert d_el.max() <= pos_tol
    assert d_az[hh >= az_h].max() <= pos_tol
    if rate is not None:
        q, q0 = rate[ok], ref_rate[ok]
        assert np.abs(q[:, 2] - q0[:, 2]).max() <= rr_tol
        # The angle rates turn with the line of sight: a position difference dp moves the horizontal direction by dp / h and so
        # changes h * (angle rate) by up to |rho_dot| dp / h -- at h = 100 km and 7 km/s, 2e-9 km/s for dp = 3e-8 km, the
        # level at which the two propagators' positions agree.  The gates take that share out (dp: this point's own position
        # difference) and hold the rest to ar_tol.  The elevation rate is scaled by h like the azimuth rate: it is singular at
        # the zenith too (dh/dt has no direction there).
        dp = np.sqrt(d_rng ** 2 + d_el ** 2 + np.minimum(daz, np.pi) ** 2 * hh ** 2)
        speed = np.sqrt(q0[:, 2] ** 2 + (q0[:, 1] * r0[:, 2]) ** 2 + (q0[:, 0] * hh) ** 2)
        with np.errstate(divide="ignore", invalid="ignore"):
            turn = np.where(hh > 0, 2.0 * speed * dp / hh, np.inf)
        sel = hh >= az_rate_h
        assert (np.abs(q[sel, 1] - q0[sel, 1]) * hh[sel] - turn[sel]).max() <= ar_tol
        assert (np.abs(q[sel, 0] - q0[sel, 0]) * hh[sel] - turn[sel]).max() <= ar_tol


def grids(start):
    rng = np.random.default_rng(3)
    exact = np.arange(0.0, 600.0, 1.0)
    jd = np.floor(start) + np.zeros(600)
    fr = (start - np.floor(start)) + np.arange(600) / 1440.0
    quasi = ((jd + fr) - start) * 1440.0  # what the (jd, fr) arithmetic hands over
    jitter = np.arange(0.0, 600.0, 1.0) + rng.uniform(-20.0, 20.0, 600) / 60.0  # +-20 s: the wide DELTA form
    random = np.sort(rng.uniform(0.0, 600.0, 300))  # the generic kernels
    return {"exact": exact, "jdfr": quasi, "jitter": jitter, "random": random}


@pytest.fixture(scope="module")
def catalog(native, orc, synth):
    pairs = synth.synth_catalog(n_near=200, n_deep=40, seed=13)
    dev = native.DeviceConstellation.from_tle_lines(pairs, 0, 0)
    cat = orc.Catalog.from_pairs(pairs, 0)
    return pairs, dev, cat


@pytest.fixture(scope="module")
def synth():
    from astroz_amd import synth as s
    return s


@pytest.mark.parametrize("grid", ["exact", "jdfr", "jitter", "random"])
@pytest.mark.parametrize("layout", ["sat_major", "time_major", "time_major_cols"])
def test_topocentric_matches_oracle(native, orc, synth, catalog, grid, layout):
    _, dev, cat = catalog
    ref = synth.START_JD + 0.25
    times = grids(ref)[grid]
    off = (ref - dev.epochs) * 1440.0
    dev.set_observer(*OBS)
    tm = layout != "sat_major"
    lay, olay = (native.TIME_MAJOR, orc.TIME_MAJOR) if tm else (native.SAT_MAJOR, orc.SAT_MAJOR)
    n, nt = dev.n, len(times)
    dev.set_tile_kernel(2 if layout == "time_major_cols" else 1)
    try:
        e0, p0, v0 = cat.propagate(times, off, mode=orc.ECEF, reference_jd=ref, layout=olay)
        ref_aer, ref_rate, h = topo_from_ecef(p0, v0, OBS)
        errT = e0.T if tm else e0
        ok = errT == 0
        for vel in (True, False):
            stride = n + 5 if tm else 0
            shape = (nt, stride, 3) if tm else (n, nt, 3)
            pos = np.full(shape, -7.0)
            v = np.full(shape, -7.0) if vel else None
            err = np.zeros((n, nt), dtype=np.uint8)
            dev.propagate_host(times, off, pos=pos, vel=v, mode=native.OUT_TOPOCENTRIC, reference_jd=ref, layout=lay,
                               stride=stride, err=err)
            assert np.array_equal(err, e0)
            if tm:
                assert (pos[:, n:] == -7.0).all()
                pos, v = pos[:, :n], (v[:, :n] if vel else None)
            gate(pos, v, ref_aer, ref_rate, h, ok)
            assert (pos[~ok] == 0.0).all()  # failing points zero-filled, as in the other frames
            if vel:
                assert (v[~ok] == 0.0).all()
        # satellite mask: masked rows untouched
        mask = (np.arange(n) % 3 != 0).astype(np.uint8)
        shape = (nt, n, 3) if tm else (n, nt, 3)
        pos = np.full(shape, -7.0)
        v = np.full(shape, -7.0)
        dev.propagate_host(times, off, pos=pos, vel=v, mode=native.OUT_TOPOCENTRIC, reference_jd=ref, layout=lay, mask=mask)
        ms = (slice(None), mask == 0) if tm else (mask == 0,)
        mk = (slice(None), mask == 1) if tm else (mask == 1,)
        assert (pos[ms] == -7.0).all() and (v[ms] == -7.0).all()
        gate(pos[mk], v[mk], ref_aer[mk], ref_rate[mk], h[mk], ok[mk])
    finally:
        dev.set_tile_kernel(1)


@pytest.mark.parametrize("layout", ["sat_major", "time_major"])
def test_topocentric_fp32(native, synth, catalog, layout):
    import torch
    _, dev, _ = catalog
    ref = synth.START_JD + 0.25
    off = (ref - dev.epochs) * 1440.0
    dev.set_observer(*OBS)
    lay = native.SAT_MAJOR if layout == "sat_major" else native.TIME_MAJOR
    for grid in ("exact", "random"):
        times = grids(ref)[grid]
        shape = (dev.n, len(times), 3) if lay == native.SAT_MAJOR else (len(times), dev.n, 3)
        p64, v64 = np.empty(shape), np.empty(shape)
        dev.propagate_host(times, off, pos=p64, vel=v64, mode=native.OUT_TOPOCENTRIC, reference_jd=ref, layout=lay)
        p32 = torch.empty(shape, dtype=torch.float32, device="cuda")
        v32 = torch.empty_like(p32)
        dev.propagate_device(times, off, p32.data_ptr(), v32.data_ptr(), mode=native.OUT_TOPOCENTRIC, reference_jd=ref,
                             layout=lay, f32=True)
        torch.cuda.synchronize()
        a, b = p32.cpu().numpy().astype(np.float64), v32.cpu().numpy().astype(np.float64)
        # fp64 arithmetic rounded once at the store: within fp32 rounding of the fp64 result
        # (the two launches may take different kernel families: their fp64 results agree to ~1e-13, hence the small slack)
        for x, y in ((a, p64), (b, v64)):
            assert (np.abs(x - y) <= np.maximum(np.abs(y) * 2.0 ** -24 * 1.01, 1e-13)).all()


def test_device_epilogue_matches_host_twin(native, synth, catalog):
    _, dev, _ = catalog
    L = native.lib()
    ref = synth.START_JD + 0.25
    off = (ref - dev.epochs) * 1440.0
    times = np.arange(0.0, 120.0, 4.0)
    n, nt = dev.n, len(times)
    dev.set_observer(*OBS)
    pt, vt = np.empty((n, nt, 3)), np.empty((n, nt, 3))
    err = np.zeros((n, nt), dtype=np.uint8)
    dev.propagate_host(times, off, pos=pt, vel=vt, layout=native.SAT_MAJOR, err=err)
    pa, va = np.empty((n, nt, 3)), np.empty((n, nt, 3))
    dev.propagate_host(times, off, pos=pa, vel=va, mode=native.OUT_TOPOCENTRIC, reference_jd=ref, layout=native.SAT_MAJOR)
    # The Greenwich angle the kernels used, read back from an ECEF run of the same grid (angle of the TEME x-y projection minus
    # that of the ECEF one): coords_julian_to_gmst evaluates GMST(jd) at jd ~ 2.46e6, where a contracted multiply-add on the
    # device and the host's separate rounding already differ by ~1e-12 rad -- 4e-8 km at GEO range, more than the gate.
    pe = np.empty((n, nt, 3))
    dev.propagate_host(times, off, pos=pe, mode=native.OUT_ECEF, reference_jd=ref, layout=native.SAT_MAJOR)
    s0 = int(np.flatnonzero((err == 0).all(axis=1) & (np.hypot(pt[:, 0, 0], pt[:, 0, 1]) > 1000.0))[0])
    gmst = np.arctan2(pt[s0, :, 1], pt[s0, :, 0]) - np.arctan2(pe[s0, :, 1], pe[s0, :, 0])
    lla = np.array(OBS)
    aer, rate = np.zeros((n, nt, 3)), np.zeros((n, nt, 3))
    for j, t in enumerate(times):
        g = float(gmst[j])
        for s in range(n):
            a3, r3 = np.zeros(3), np.zeros(3)
            rs, vs = np.ascontiguousarray(pt[s, j]), np.ascontiguousarray(vt[s, j])
            L.azh_coords_topocentric(rs.ctypes.data, vs.ctypes.data, g, lla.ctypes.data, a3.ctypes.data, r3.ctypes.data)
            aer[s, j], rate[s, j] = a3, r3
    h = aer[..., 2] * np.cos(aer[..., 1])
    ok = err == 0
    gate(pa, va, aer, rate, h, ok, pos_tol=1e-9, rr_tol=1e-11, ar_tol=1e-11, az_rate_h=100.0, az_h=1.0)


def test_observer_argument_checks(native, synth):
    L = native.lib()
    pairs = synth.synth_catalog(n_near=10, seed=5)
    dev = native.DeviceConstellation.from_tle_lines(pairs, 0, 0)
    times = np.arange(0.0, 10.0)
    pos = np.empty((len(times), dev.n, 3))
    assert L.azh_propagate_host(dev._h, times.ctypes.data, len(times), None, pos.ctypes.data, None, 3, synth.START_JD,
                                None, native.TIME_MAJOR, 0, None) == -20  # no observer yet
    for bad in ((90.5, 0.0, 0.0), (-91.0, 0.0, 0.0), (np.nan, 0.0, 0.0), (0.0, np.inf, 0.0), (0.0, 0.0, np.nan)):
        assert L.azh_set_observer(dev._h, *bad) == -20
    assert L.azh_propagate_host(dev._h, times.ctypes.data, len(times), None, pos.ctypes.data, None, 3, synth.START_JD,
                                None, native.TIME_MAJOR, 0, None) == -20  # (still none: rejected input changes nothing)
    assert L.azh_propagate_host(dev._h, times.ctypes.data, len(times), None, pos.ctypes.data, None, 4, synth.START_JD,
                                None, native.TIME_MAJOR, 0, None) == -20
    out = np.zeros(4, dtype=native.PASS_DTYPE)
    cnt = np.zeros(dev.n, dtype=np.uint32)
    assert L.azh_find_passes_host(dev._h, times.ctypes.data, len(times), None, 0.0, 10.0, out.ctypes.data, 0,
                                  cnt.ctypes.data) == -20  # no observer
    dev.set_observer(0.0, 0.0, 0.0)
    for bad_t in (np.array([0.0, 1.0, 1.0, 2.0]), np.array([0.0, 2.0, 1.0]), np.array([0.0, np.nan, 2.0])):
        assert L.azh_find_passes_host(dev._h, bad_t.ctypes.data, len(bad_t), None, 0.0, 10.0, out.ctypes.data, 0,
                                      cnt.ctypes.data) == -20
    with pytest.raises(native.NativeError):
        dev.set_observer(100.0, 0.0, 0.0)


def test_set_observer_between_cached_launches(native, synth):
    import torch
    pairs = synth.synth_catalog(n_near=3000, n_deep=20, seed=21)
    dev = native.DeviceConstellation.from_tle_lines(pairs, 0, 0)
    ref = synth.START_JD
    off = (ref - dev.epochs) * 1440.0
    times = np.arange(0.0, 256.0)
    shape = (len(times), dev.n, 3)
    p = torch.empty(shape, dtype=torch.float64, device="cuda")
    v = torch.empty_like(p)
    host = {}
    for o in ((10.0, 20.0, 0.0), (-35.0, 150.0, 1.0)):
        a, b = np.empty(shape), np.empty(shape)
        dev.set_observer(*o)
        dev.propagate_host(times, off, pos=a, vel=b, mode=native.OUT_TOPOCENTRIC, reference_jd=ref)
        host[o] = (a, b)
    for graphs in (0, 1):
        dev.set_graphs(graphs)
        dev.set_observer(10.0, 20.0, 0.0)
        dev.propagate_device(times, off, p.data_ptr(), v.data_ptr(), mode=native.OUT_TOPOCENTRIC, reference_jd=ref)
        for k in range(6):  # eager, captured, replayed ... then a new observer, then back
            o = (10.0, 20.0, 0.0) if k in (0, 1, 2, 5) else (-35.0, 150.0, 1.0)
            if k in (3, 5):
                dev.set_observer(*o)
            dev.propagate_device_cached(p.data_ptr(), v.data_ptr())
            torch.cuda.synchronize()
            a, b = host[o]
            assert np.array_equal(p.cpu().numpy(), a), (graphs, k)
            assert np.array_equal(v.cpu().numpy(), b), (graphs, k)
    dev.set_graphs(0)


# ---- passes -------------------------------------------------------------------------------------------------------

def _herm(f0, f1, m0, m1, s):
    s2 = s * s
    s3 = s2 * s
    return (2 * s3 - 3 * s2 + 1) * f0 + (s3 - 2 * s2 + s) * m0 + (3 * s2 - 2 * s3) * f1 + (s3 - s2) * m1


def _herm_d(f0, f1, m0, m1, s):
    return (6 * s * s - 6 * s) * (f0 - f1) + (3 * s * s - 4 * s + 1) * m0 + (3 * s * s - 2 * s) * m1


def _root(f0, f1, m0, m1):
    g = lambda s: _herm(f0, f1, m0, m1, s)  # noqa: E731
    dg = lambda s: _herm_d(f0, f1, m0, m1, s)  # noqa: E731
    g0, g1 = f0, f1
    if g0 == 0.0:
        return 0.0
    if g1 == 0.0:
        return 1.0
    lo, hi, s = 0.0, 1.0, g0 / (g0 - g1)
    for _ in range(64):
        gs = g(s)
        if gs == 0.0:
            break
        if (gs < 0.0) == (g0 < 0.0):
            lo = s
        else:
            hi = s
        d = dg(s)
        sn = s - gs / d if d != 0.0 else lo
        if not (lo < sn < hi):
            sn = 0.5 * (lo + hi)
        done = abs(sn - s) <= 1e-15
        s = sn
        if done:
            break
    return s


def _enu_state(p, v):
    se, ce, sa, ca = np.sin(p[1]), np.cos(p[1]), np.sin(p[0]), np.cos(p[0])
    h, hd = p[2] * ce, v[2] * ce - p[2] * se * v[1]
    return [(h * sa, hd * sa + h * ca * v[0]), (h * ca, hd * ca - h * sa * v[0]), (p[2] * se, v[2] * se + p[2] * ce * v[1])]


def _culmination(p0, v0, p1, v1, dt):
    """Highest point of the Hermite-interpolated ENU track on [t0, t1]: (s, elevation); regula falsi (Illinois) on the sign
    of the elevation's derivative, as k_passes."""
    a, b, k = _enu_state(p0, v0), _enu_state(p1, v1), 60.0 * dt

    def track(s):
        x = [_herm(a[j][0], b[j][0], k * a[j][1], k * b[j][1], s) for j in range(3)]
        xd = [_herm_d(a[j][0], b[j][0], k * a[j][1], k * b[j][1], s) for j in range(3)]
        return x, xd

    def slope(s):
        x, xd = track(s)
        return (x[0] * x[0] + x[1] * x[1]) * xd[2] - x[2] * (x[0] * xd[0] + x[1] * xd[1])
    lo, hi, g_lo, g_hi, s, side = 0.0, 1.0, slope(0.0), slope(1.0), 0.5, 0
    for _ in range(40):
        if not (g_lo > 0.0 and g_hi < 0.0):
            break
        sn = (lo * g_hi - hi * g_lo) / (g_hi - g_lo)
        done = abs(sn - s) <= 1e-14
        s = sn
        gs = slope(s)
        if done or gs == 0.0:
            break
        if gs > 0.0:
            lo, g_lo = s, gs
            if side == 1:
                g_hi *= 0.5
            side = 1
        else:
            hi, g_hi = s, gs
            if side == -1:
                g_lo *= 0.5
            side = -1
    x, _ = track(s)
    return s, np.arctan2(x[2], np.hypot(x[0], x[1]))


def _azimuth(a0, a1, m0, m1, s):
    d = a1 - a0
    d -= 2 * np.pi * np.rint(d / (2 * np.pi))
    a = _herm(a0, a0 + d, m0, m1, s)
    return a - 2 * np.pi * np.floor(a / (2 * np.pi))


def scan_passes(times, P, V, E, min_el):
    """The grid-level algorithm of k_passes, here in numpy / Python, on one satellite's topocentric row."""
    n = len(times)
    up = (E == 0) & (P[:, 1] >= min_el)
    bad = E != 0
    out = []
    i = 0
    while i < n:
        if not up[i]:
            i += 1
            continue
        j = i
        while j + 1 < n and up[j + 1]:
            j += 1
        flags = 0
        if i == 0:
            t_r, az_r, flags = times[0], P[0, 0], 1
        elif bad[i - 1]:
            t_r, az_r, flags = times[i], P[i, 0], 4
        else:
            dt = times[i] - times[i - 1]
            s = _root(P[i - 1, 1] - min_el, P[i, 1] - min_el, 60 * dt * V[i - 1, 1], 60 * dt * V[i, 1])
            t_r, az_r = s * dt + times[i - 1], _azimuth(P[i - 1, 0], P[i, 0], 60 * dt * V[i - 1, 0], 60 * dt * V[i, 0], s)
        if j == n - 1:
            t_s, az_s, flags = times[n - 1], P[n - 1, 0], flags | 2
        elif bad[j + 1]:
            t_s, az_s, flags = times[j], P[j, 0], flags | 4
        else:
            dt = times[j + 1] - times[j]
            s = _root(P[j, 1] - min_el, P[j + 1, 1] - min_el, 60 * dt * V[j, 1], 60 * dt * V[j + 1, 1])
            t_s, az_s = s * dt + times[j], _azimuth(P[j, 0], P[j + 1, 0], 60 * dt * V[j, 0], 60 * dt * V[j + 1, 0], s)
        k = i + int(np.argmax(P[i:j + 1, 1]))
        t_c, e_c = times[k], P[k, 1]
        for i0 in (k - 1, k):
            i1 = i0 + 1
            if i0 < 0 or i1 >= n or E[i0] or E[i1]:
                continue
            d0, d1 = V[i0, 1], V[i1, 1]
            if not (d0 > 0 and d1 < 0):
                continue
            dt = times[i1] - times[i0]
            s, e = _culmination(P[i0], V[i0], P[i1], V[i1], dt)
            if e > e_c:
                e_c, t_c = e, s * dt + times[i0]
        out.append(dict(t_rise_min=t_r, t_culm_min=t_c, t_set_min=t_s, max_elevation_rad=e_c, rise_azimuth_rad=az_r,
                        set_azimuth_rad=az_s, flags=flags, grid_rise=i, grid_culm=k, grid_set=j))
        i = j + 1
    return out


@pytest.fixture(scope="module")
def pass_case(native, synth):
    pairs = synth.synth_catalog(n_near=197, n_deep=3, seed=41)
    # one eccentric member and one geostationary member 10 degrees east of the observer (right ascension = GMST + longitude)
    gmst = np.degrees(native.lib().coords_julian_to_gmst(synth.START_JD))
    pairs.append(synth.format_tle(99001, synth.START_JD, 63.4, 40.0, 0.25, 270.0, 10.0, 9.0, 1e-5))
    pairs.append(synth.format_tle(99002, synth.START_JD, 0.05, (gmst + OBS[1] + 10.0) % 360.0, 0.0002, 0.0, 0.0, 1.00273791, 0.0))
    dev = native.DeviceConstellation.from_tle_lines(pairs, 0, 0)
    ref = synth.START_JD
    off = (ref - dev.epochs) * 1440.0
    times = np.arange(0.0, 1440.0)
    dev.set_observer(*OBS)
    rec, cnt = dev.find_passes(times, off, reference_jd=ref, min_elevation_deg=10.0, max_passes=32)
    return pairs, dev, ref, off, times, rec, cnt


def test_passes_match_grid_algorithm(native, pass_case):
    pairs, dev, ref, off, times, rec, cnt = pass_case
    n, nt = dev.n, len(times)
    P, V = np.empty((n, nt, 3)), np.empty((n, nt, 3))
    E = np.zeros((n, nt), dtype=np.uint8)
    dev.propagate_host(times, off, pos=P, vel=V, mode=native.OUT_TOPOCENTRIC, reference_jd=ref, layout=native.SAT_MAJOR,
                       err=E)
    min_el = np.radians(10.0)
    total = 0
    for s in range(n):
        want = scan_passes(times, P[s], V[s], E[s], min_el)
        assert cnt[s] == len(want), s
        total += len(want)
        for k, w in enumerate(want):
            g = rec[s, k]
            for f in ("flags", "grid_rise", "grid_culm", "grid_set"):
                assert int(g[f]) == w[f], (s, k, f)
            for f in ("t_rise_min", "t_culm_min", "t_set_min"):
                # (the top of a pass that lasts hours -- the geostationary member's -- is flat: its time is ill-conditioned)
                tol = 1e-9 if f != "t_culm_min" or w["t_set_min"] - w["t_rise_min"] < 60.0 else 1e-6
                assert abs(float(g[f]) - w[f]) <= tol, (s, k, f, float(g[f]), w[f])
            assert abs(float(g["max_elevation_rad"]) - w["max_elevation_rad"]) <= 1e-10
            for f in ("rise_azimuth_rad", "set_azimuth_rad"):
                d = (float(g[f]) - w[f] + np.pi) % (2 * np.pi) - np.pi
                assert abs(d) <= 1e-9 and 0.0 <= float(g[f]) < 2 * np.pi
    assert total > 100
    assert (rec["flags"][:, :] & native.PASS_UP_AT_START).any() and (rec["flags"] & native.PASS_UP_AT_END).any()
    geo = n - 1
    assert cnt[geo] == 1 and int(rec[geo, 0]["flags"]) == 3  # the geostationary member: up all day
    assert rec[geo, 0]["t_rise_min"] == times[0] and rec[geo, 0]["t_set_min"] == times[-1]


def test_passes_against_one_second_scan(native, orc, pass_case):
    pairs, dev, ref, off, times, rec, cnt = pass_case
    cat = orc.Catalog.from_pairs(pairs, 0)
    min_el = np.radians(10.0)
    fine = np.arange(0.0, times[-1] * 60.0 + 0.5) / 60.0  # every second
    matched = 0
    for lo in range(0, dev.n, 25):
        hi = min(dev.n, lo + 25)
        sub = orc.Catalog.from_pairs(pairs[lo:hi], 0)
        e0, p0, _ = sub.propagate(fine, off[lo:hi], velocities=False, mode=orc.ECEF, reference_jd=ref, threads=16)
        for s in range(lo, hi):
            aer, _, _ = topo_from_ecef(p0[s - lo], None, OBS)
            el = aer[:, 1]
            up = (e0[s - lo] == 0) & (el >= min_el)
            d = np.diff(up.astype(np.int8))
            starts = list(np.flatnonzero(d == 1) + 1)
            ends = list(np.flatnonzero(d == -1))
            if up[0]:
                starts.insert(0, 0)
            if up[-1]:
                ends.append(len(up) - 1)
            truth = []
            for a, b in zip(starts, ends):
                # sub-second rise / set: linear between the bracketing seconds
                tr = fine[a] if a == 0 else fine[a - 1] + (min_el - el[a - 1]) / (el[a] - el[a - 1]) / 60.0
                ts = fine[b] if b == len(up) - 1 else fine[b] + (el[b] - min_el) / (el[b] - el[b + 1]) / 60.0
                k = a + int(np.argmax(el[a:b + 1]))
                tk, ek = fine[k], el[k]
                if a < k < b:  # the top between the samples: parabola through the three around the sampled maximum
                    c2 = el[k - 1] - 2 * el[k] + el[k + 1]
                    if c2 < 0:
                        u = 0.5 * (el[k - 1] - el[k + 1]) / c2
                        tk, ek = tk + u / 60.0, el[k] - 0.25 * (el[k - 1] - el[k + 1]) * u
                truth.append((tr, tk, ts, ek, a == 0 or b == len(up) - 1))
            got = rec[s, :min(int(cnt[s]), rec.shape[1])]
            for g in got:
                m = [t for t in truth if t[0] - 1.0 / 60 <= g["t_culm_min"] <= t[2] + 1.0 / 60]
                assert len(m) == 1, (s, g)
                tr, tc, ts, emax, open_end = m[0]
                assert abs(g["t_rise_min"] - tr) * 60.0 <= 2.0, (s, g["t_rise_min"], tr)
                assert abs(g["t_set_min"] - ts) * 60.0 <= 2.0, (s, g["t_set_min"], ts)
                assert abs(g["max_elevation_rad"] - emax) <= (1e-3 if emax > np.radians(85.0) else 1e-4), (s, g, emax)
                # (culmination time: passes of LEO-like duration; over an apogee dwell the elevation is flat for minutes)
                if not open_end and ts - tr < 60.0:
                    assert abs(g["t_culm_min"] - tc) * 60.0 <= 10.0, (s, g["t_culm_min"], tc)
                matched += 1
            for t in truth:
                if t[3] >= min_el + np.radians(0.5):
                    assert any(g["t_rise_min"] <= t[1] <= g["t_set_min"] for g in got), (s, t)
    assert matched == int(cnt.sum()) and matched > 100


def test_pass_edge_cases(native, synth, pass_case):
    import torch
    pairs, dev, ref, off, times, rec, cnt = pass_case
    # room for fewer records than there are passes: the first ones, and the true count
    r1, c1 = dev.find_passes(times, off, reference_jd=ref, min_elevation_deg=10.0, max_passes=1)
    assert np.array_equal(c1, cnt)
    has = cnt > 0
    assert r1[has, 0].tobytes() == rec[has, 0].tobytes()
    r0, c0 = dev.find_passes(times, off, reference_jd=ref, min_elevation_deg=10.0, max_passes=0)
    assert np.array_equal(c0, cnt)
    # _host and _device give identical records
    mp = rec.shape[1]
    d_out = torch.zeros(dev.n * mp * 64, dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(dev.n, dtype=torch.int32, device="cuda")
    dev.find_passes_device(times, off, d_out.data_ptr(), mp, d_n.data_ptr(), reference_jd=ref, min_elevation_deg=10.0)
    torch.cuda.synchronize()
    assert np.array_equal(d_n.cpu().numpy().astype(np.uint32), cnt)
    got = d_out.cpu().numpy().view(native.PASS_DTYPE).reshape(dev.n, mp)
    for s in range(dev.n):
        k = min(int(cnt[s]), mp)
        assert got[s, :k].tobytes() == rec[s, :k].tobytes()
    # a satellite whose propagation fails mid-grid (perigee inside the Earth near some perigee passages): an observer right
    # under it at the grid point before its first failure sees a pass cut by that error
    bad = synth.format_tle(99100, synth.START_JD, 63.4, 10.0, 0.49, 270.0, 0.0, 6.1, 0.01)
    one = native.DeviceConstellation.from_tle_lines([bad], 0, 0)
    t = np.arange(0.0, 1440.0)
    e = np.zeros((1, len(t)), dtype=np.uint8)
    p = np.empty((1, len(t), 3))
    one.propagate_host(t, None, pos=p, err=e, mode=native.OUT_ECEF, reference_jd=synth.START_JD, layout=native.SAT_MAJOR)
    first = int(np.flatnonzero(e[0])[0])
    assert 10 < first < len(t) - 10 and not e[0, :first].any()
    lla = np.zeros(3)
    x = np.ascontiguousarray(p[0, first - 1])
    native.lib().coords_ecef_to_geodetic(x.ctypes.data, lla.ctypes.data)
    one.set_observer(lla[0], lla[1], lla[2] - 5.0)
    rr, cc = one.find_passes(t, None, reference_jd=synth.START_JD, min_elevation_deg=10.0, max_passes=64)
    cut = [g for g in rr[0, :int(cc[0])] if g["grid_set"] == first - 1]
    assert len(cut) == 1 and int(cut[0]["flags"]) & native.PASS_CUT_BY_ERROR
    assert cut[0]["t_set_min"] == t[first - 1]


def test_python_end_to_end(native, synth):
    import astroz_amd
    pairs = synth.synth_catalog(n_near=40, seed=77)
    text = synth.pairs_to_text(pairs)
    const = astroz_amd.Constellation(text)
    when = datetime.fromtimestamp((synth.START_JD - 2440587.5) * 86400.0, tz=timezone.utc)
    start = astroz_amd._jd_of(when)
    times = np.arange(0.0, 1440.0)
    aer, rates = astroz_amd.propagate(const, times, start_time=when, output="topocentric", observer=OBS, velocities=True)
    assert aer.shape == (len(times), const.num_satellites, 3) and rates.shape == aer.shape
    e = astroz_amd.propagate(const, times, start_time=when, output="ecef", velocities=True)
    ref_aer, ref_rate, h = topo_from_ecef(e[0], e[1], OBS)
    gate(aer, rates, ref_aer, ref_rate, h, np.ones(h.shape, dtype=bool))
    with pytest.raises(ValueError):
        astroz_amd.propagate(const, times, start_time=when, output="topocentric")
    with pytest.raises(ValueError):
        astroz_amd.propagate(const, times, start_time=when, output="ecef", observer=OBS)
    with pytest.raises(ValueError):
        astroz_amd.propagate(const, times, start_time=when, output="nope")
    ps = astroz_amd.passes(const, times, OBS, min_elevation=10.0, start_time=when)
    assert ps.dtype.names == ("sat", "rise", "culmination", "set", "max_elevation", "rise_azimuth", "set_azimuth", "flags")
    assert len(ps) > 20
    key = ps["sat"].astype(np.float64) * 1e6 + ps["rise"]
    assert (np.diff(key) > 0).all()  # sorted by (sat, rise)
    assert (ps["rise"] <= ps["culmination"]).all() and (ps["culmination"] <= ps["set"]).all()
    assert (ps["max_elevation"] >= np.radians(10.0)).all()
    # the same passes from the native call
    const._dev.set_observer(*OBS)
    rec, cnt = const._dev.find_passes(times, (start - const._dev.epochs) * 1440.0, reference_jd=start, max_passes=64)
    assert len(ps) == int(cnt.sum())
    # overflow: more passes per satellite than the wrapper's first guess of room (a 0-degree mask over 3 days)
    long_t = np.arange(0.0, 3 * 1440.0)
    ps0 = astroz_amd.passes(const, long_t, OBS, min_elevation=0.0, start_time=when)
    const._dev.set_observer(*OBS)
    rec0, cnt0 = const._dev.find_passes(long_t, (start - const._dev.epochs) * 1440.0, reference_jd=start, min_elevation_deg=0.0,
                                        max_passes=256)
    assert int(cnt0.max()) > 16 and len(ps0) == int(cnt0.sum())
    assert np.array_equal(ps0["rise"], np.concatenate([rec0[s, :cnt0[s]]["t_rise_min"] for s in range(len(cnt0))]))
    # Sgp4Constellation.propagate_into gains the same mode
    sc = astroz_amd.Sgp4Constellation.from_tle_text(text)
    out = np.empty((len(times), sc.num_satellites, 3))
    sc.propagate_into(times, out, epoch_offsets=(start - np.array(sc.epochs)) * 1440.0, output="topocentric", observer=OBS,
                      reference_jd=start)
    assert np.abs(out - aer).max() < 1e-9
