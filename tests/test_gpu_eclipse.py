"""Earth-shadow intervals on the GPU (azh_find_eclipses_*, astroz_amd.eclipses): the device Sun against its host twin, the
kernel against a numpy restatement of its grid algorithm, against an independent one-second scan of the oracle propagator,
geostationary and dawn-dusk members in and out of their eclipse seasons, the edge cases of the pass finder, and the Python
entry point.  The Sun and shadow formulas are restated here in numpy; the reference project has nothing to compare with."""
from datetime import datetime, timezone

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

AU = 149597870.7
R_EARTH, R_SUN = 6378.137, 696000.0
VALUE, NULL = -20, -101


@pytest.fixture(scope="module")
def synth():
    from astroz_amd import synth as s
    return s


# ---- the model in numpy ---------------------------------------------------------------------------------------------

def numpy_sun(jd):
    """The low-precision Almanac series (Vallado, algorithm "Sun"): km, mean equator of date used as TEME."""
    jd = np.asarray(jd, dtype=np.float64)
    T = (jd - 2451545.0) / 36525.0
    lam_m = np.mod(280.460 + 36000.771 * T, 360.0)
    M = np.radians(np.mod(357.5291092 + 35999.05034 * T, 360.0))
    lam = np.radians(lam_m + 1.914666471 * np.sin(M) + 0.019994643 * np.sin(2 * M))
    r = 1.000140612 - 0.016708617 * np.cos(M) - 0.000139589 * np.cos(2 * M)
    eps = np.radians(23.439291 - 0.0130042 * T)
    return AU * np.stack([r * np.cos(lam), r * np.cos(eps) * np.sin(lam), r * np.sin(eps) * np.sin(lam)], axis=-1)


def sun_table(sun):
    """(unit vector (n, 3), tan a_u (n,), tan a_p (n,)) of Sun vectors (n, 3) km."""
    d = np.linalg.norm(sun, axis=-1)
    su, sp = (R_SUN - R_EARTH) / d, (R_SUN + R_EARTH) / d
    return sun / d[..., None], su / np.sqrt(1 - su * su), sp / np.sqrt(1 - sp * sp)


def shadow(P, tab):
    """x, h, f_umbra, f_penumbra of positions P (..., n, 3) against the table of their n times."""
    s, tu, tp = tab
    x = -(P * s).sum(-1)
    h = np.linalg.norm(np.cross(P, s), axis=-1)
    return x, h, h - (R_EARTH - x * tu), h - (R_EARTH + x * tp)


def states(P, E, tab):
    x, h, fu, fp = shadow(P, tab)
    st = np.where(x > 0, np.where(fu < 0, 2, np.where(fp < 0, 1, 0)), 0).astype(np.uint8)
    st[E != 0] = 255
    return st, fu, fp


def _herm(f0, f1, m0, m1, s):
    s2 = s * s
    s3 = s2 * s
    return (2 * s3 - 3 * s2 + 1) * f0 + (s3 - 2 * s2 + s) * m0 + (3 * s2 - 2 * s3) * f1 + (s3 - s2) * m1


def _herm_d(f0, f1, m0, m1, s):
    return (6 * s * s - 6 * s) * (f0 - f1) + (3 * s * s - 4 * s + 1) * m0 + (3 * s * s - 2 * s) * m1


def _root(f0, f1, m0, m1):
    """az_herm_root: safeguarded Newton from the linear estimate."""
    if f0 == 0.0:
        return 0.0
    if f1 == 0.0:
        return 1.0
    lo, hi, s = 0.0, 1.0, f0 / (f0 - f1)
    for _ in range(64):
        gs = _herm(f0, f1, m0, m1, s)
        if gs == 0.0:
            break
        if (gs < 0.0) == (f0 < 0.0):
            lo = s
        else:
            hi = s
        d = _herm_d(f0, f1, m0, m1, s)
        sn = s - gs / d if d != 0.0 else lo
        if not (lo < sn < hi):
            sn = 0.5 * (lo + hi)
        done = abs(sn - s) <= 1e-15
        s = sn
        if done:
            break
    return s


def _g(r, v, s, sd, tu, tp, penumbra, k):
    """g = max(f, -x) and 60 dt dg/dt at one end of an interval; sd = the rate of the Sun direction over it (per second)."""
    x = -np.dot(r, s)
    h = np.linalg.norm(np.cross(r, s))
    xd = -np.dot(v, s) - np.dot(r, sd)
    hd = (np.dot(r, v) - x * xd) / h if h > 0 else 0.0
    f, fd = (h - (R_EARTH + x * tp), hd - xd * tp) if penumbra else (h - (R_EARTH - x * tu), hd + xd * tu)
    return (f, k * fd) if f >= -x else (-x, -k * xd)


def scan_eclipses(times, P, V, E, tab, penumbra):
    """The grid-level algorithm of k_eclipses, here in numpy / Python, on one satellite's TEME row."""
    n = len(times)
    st, _, _ = states(P, E, tab)
    inn = (st == 2) | ((st == 1) & bool(penumbra))
    bad = E != 0
    s, tu, tp = tab

    def refine(i0):
        i1 = i0 + 1
        dt = times[i1] - times[i0]
        k = 60.0 * dt
        sd = (s[i1] - s[i0]) / k
        g0, m0 = _g(P[i0], V[i0], s[i0], sd, tu[i0], tp[i0], penumbra, k)
        g1, m1 = _g(P[i1], V[i1], s[i1], sd, tu[i1], tp[i1], penumbra, k)
        return _root(g0, g1, m0, m1) * dt + times[i0]
    out = []
    i = 0
    while i < n:
        if not inn[i]:
            i += 1
            continue
        j = i
        while j + 1 < n and inn[j + 1]:
            j += 1
        flags = 0
        if i == 0:
            t_in, flags = times[0], 1
        elif bad[i - 1]:
            t_in, flags = times[i], 4
        else:
            t_in = refine(i - 1)
        if j == n - 1:
            t_out, flags = times[n - 1], flags | 2
        elif bad[j + 1]:
            t_out, flags = times[j], flags | 4
        else:
            t_out = refine(j)
        out.append(dict(t_entry_min=t_in, t_exit_min=t_out, flags=flags, grid_entry=i, grid_exit=j))
        i = j + 1
    return out


def true_intervals(fine, inn, f):
    """Maximal runs of `inn` on the one-second axis `fine` (minutes): (start, end, first index, last index), the crossings
    placed linearly between the bracketing seconds of f."""
    d = np.diff(inn.astype(np.int8))
    starts = list(np.flatnonzero(d == 1) + 1)
    ends = list(np.flatnonzero(d == -1))
    if inn[0]:
        starts.insert(0, 0)
    if inn[-1]:
        ends.append(len(inn) - 1)
    out = []
    for a, b in zip(starts, ends):
        ta = fine[a] if a == 0 else fine[a - 1] + f[a - 1] / (f[a - 1] - f[a]) / 60.0
        tb = fine[b] if b == len(inn) - 1 else fine[b] + f[b] / (f[b] - f[b + 1]) / 60.0
        out.append((ta, tb, a, b))
    return out


# ---- the catalog of the grid and oracle checks -------------------------------------------------------------------------

def eclipse_pairs(synth):
    """About 200 synthetic near-earth rows, the three reference deep-space members, one eccentric member and one
    geostationary member (test_gpu_topocentric's pass catalog, the geostationary member at right ascension 0)."""
    pairs = synth.synth_catalog(n_near=197, n_deep=3, seed=41)
    pairs.append(synth.format_tle(99001, synth.START_JD, 63.4, 40.0, 0.25, 270.0, 10.0, 9.0, 1e-5))
    pairs.append(synth.format_tle(99002, synth.START_JD, 0.05, 0.0, 0.0002, 0.0, 0.0, 1.00273791, 0.0))
    return pairs


@pytest.fixture(scope="module")
def case(native, synth):
    pairs = eclipse_pairs(synth)
    dev = native.DeviceConstellation.from_tle_lines(pairs, 0, 0)
    ref = synth.START_JD
    off = (ref - dev.epochs) * 1440.0
    times = np.arange(0.0, 1440.0)
    res = {kind: dev.find_eclipses(times, off, reference_jd=ref, kind=kind, max_eclipses=32, state=True) for kind in (0, 1)}
    return pairs, dev, ref, off, times, res


def test_device_sun_matches_host_twin(native):
    """Both twins are the same few fp64 operations (one source); they differ in sin / cos (libm against az_sincos, about an
    ulp each) and in the contraction of multiply-adds."""
    rng = np.random.default_rng(5)
    jd = np.concatenate([[2453827.5], rng.uniform(2433282.5, 2469807.5, 9999)])  # 1950 .. 2050
    host = native.sun_position(jd)
    devs = native.selftest_sun(jd)
    rel = np.linalg.norm(devs - host, axis=1) / np.linalg.norm(host, axis=1)
    print("device Sun vs host twin on %d dates: max relative difference %.3g" % (len(jd), rel.max()))
    assert rel.max() <= 1e-12
    assert np.abs(devs[0] / AU - [0.9771945, 0.1924424, 0.0834308]).max() <= 5e-6  # Vallado, example 5-1
    assert (np.linalg.norm(numpy_sun(jd) - devs, axis=1) / np.linalg.norm(host, axis=1)).max() <= 1e-9


def test_eclipses_match_grid_algorithm(native, case):
    pairs, dev, ref, off, times, res = case
    n, nt = dev.n, len(times)
    P, V = np.empty((n, nt, 3)), np.empty((n, nt, 3))
    E = np.zeros((n, nt), dtype=np.uint8)
    dev.propagate_host(times, off, pos=P, vel=V, mode=native.OUT_TEME, reference_jd=ref, layout=native.SAT_MAJOR, err=E)
    tab = sun_table(native.sun_position(ref + times / 1440.0))
    want_state, fu, fp = states(P, E, tab)
    near_edge = (np.minimum(np.abs(fu), np.abs(fp)) < 1e-9) & (E == 0)
    print("grid points with |f| < 1e-9 km: %d" % int(near_edge.sum()))
    for kind in (0, 1):
        rec, cnt, state = res[kind]
        assert state.dtype == np.uint8 and state.shape == (n, nt)
        assert np.array_equal(state[~near_edge], want_state[~near_edge])
        total, worst = 0, 0.0
        for s in range(n):
            want = scan_eclipses(times, P[s], V[s], E[s], (tab[0], tab[1], tab[2]), kind)
            assert cnt[s] == len(want), (kind, s, int(cnt[s]), len(want))
            total += len(want)
            for k, w in enumerate(want):
                g = rec[s, k]
                for f in ("flags", "grid_entry", "grid_exit"):
                    assert int(g[f]) == w[f], (kind, s, k, f)
                assert int(g["reserved"]) == 0
                for f in ("t_entry_min", "t_exit_min"):
                    worst = max(worst, abs(float(g[f]) - w[f]))
                    assert abs(float(g[f]) - w[f]) <= 1e-9, (kind, s, k, f, float(g[f]), w[f])
        print("kind %d: %d intervals, max |dt| against the numpy scan %.3g min" % (kind, total, worst))
        assert total > 2000  # about 15 a day for each near-earth row
        assert (rec["flags"] & native.ECLIPSE_IN_AT_START).any() and (rec["flags"] & native.ECLIPSE_IN_AT_END).any()
    # any shadow contains the umbra
    assert ((res[1][2] >= 1) >= (res[0][2] == 2)).all() and np.array_equal(res[0][2], res[1][2])


def test_eclipses_against_one_second_scan(native, orc, case):
    """Every reported interval is one true interval of the oracle's one-second scan; a refined end lies within 2 s of the
    truth, or the oracle's f there is within 1 km of zero (grazing crossings).  True intervals without a grid point are out
    of a grid scan's reach: 0 of 2,684 (umbra) and 1 of 2,693 (any shadow) in this catalog on this date, measured with the oracle alone."""
    pairs, dev, ref, off, times, res = case
    fine = np.arange(0.0, times[-1] * 60.0 + 0.5) / 60.0  # every second
    tab = sun_table(numpy_sun(ref + fine / 1440.0))
    for kind in (0, 1):
        rec, cnt, _ = res[kind]
        assert not (rec["flags"] & native.ECLIPSE_CUT_BY_ERROR).any()
    n_true, n_unseen, matched = [0, 0], [0, 0], [0, 0]
    worst = [0.0, 0.0]
    for lo in range(0, dev.n, 25):
        hi = min(dev.n, lo + 25)
        sub = orc.Catalog.from_pairs(pairs[lo:hi], 0)
        e0, p0, _ = sub.propagate(fine, off[lo:hi], velocities=False, mode=orc.TEME, reference_jd=ref, threads=16)
        assert not e0.any()
        x, h, fu, fp = shadow(p0, tab)
        for kind in (0, 1):
            rec, cnt, _ = res[kind]
            fk = fp if kind else fu
            for s in range(lo, hi):
                f = fk[s - lo]
                truth = true_intervals(fine, (x[s - lo] > 0) & (f < 0), f)
                got = rec[s, :min(int(cnt[s]), rec.shape[1])]
                assert int(cnt[s]) <= rec.shape[1]
                used = set()
                for g in got:
                    anchor = times[int(g["grid_entry"])]  # a grid time inside the reported interval
                    m = [q for q, t in enumerate(truth) if t[0] - 1.0 / 60 <= anchor <= t[1] + 1.0 / 60]
                    assert len(m) == 1 and m[0] not in used, (kind, s, g, m)
                    used.add(m[0])
                    ta, tb, a, b = truth[m[0]]
                    for t_rep, t_true in ((float(g["t_entry_min"]), ta), (float(g["t_exit_min"]), tb)):
                        dt_s = abs(t_rep - t_true) * 60.0
                        f_there = abs(float(np.interp(t_rep, fine, f)))
                        assert dt_s <= 2.0 or f_there <= 1.0, (kind, s, g, t_true, dt_s, f_there)
                        if dt_s <= 2.0:
                            worst[kind] = max(worst[kind], dt_s)
                    matched[kind] += 1
                for q, (ta, tb, a, b) in enumerate(truth):
                    n_true[kind] += 1
                    if (b // 60) * 60 >= a:  # holds a grid point (the whole minutes): it must have been found
                        k = b // 60
                        assert any(int(g["grid_entry"]) <= k <= int(g["grid_exit"]) for g in got), (kind, s, ta, tb)
                    else:
                        n_unseen[kind] += 1
    for kind in (0, 1):
        print("kind %d: %d true intervals, %d without a grid point, %d matched, max |dt| %.4f s" %
              (kind, n_true[kind], n_unseen[kind], matched[kind], worst[kind]))
        assert matched[kind] == int(res[kind][1].sum()) and matched[kind] > 2000
        assert n_unseen[kind] <= 0.02 * n_true[kind]


def _jd(y, m, d):
    return datetime(y, m, d, tzinfo=timezone.utc).timestamp() / 86400.0 + 2440587.5


def test_eclipse_seasons(native, synth):
    times = np.arange(0.0, 1440.0)
    # a geostationary member: one eclipse of roughly an hour a day inside the equinox season, none near a solstice
    # (at the Sun's right ascension at the first grid time -- local noon -- so that its midnight falls in the middle of the day)
    for jd, in_season in ((_jd(2025, 3, 20), True), (_jd(2025, 9, 23), True), (_jd(2025, 6, 21), False), (_jd(2025, 12, 21), False)):
        sun = native.sun_position(jd)
        geo = synth.format_tle(99002, jd, 0.05, 0.0, 0.0002, 0.0, np.degrees(np.arctan2(sun[1], sun[0])) % 360.0, 1.00273791, 0.0)
        dev = native.DeviceConstellation.from_tle_lines([geo], 0, 0)
        for kind in (0, 1):
            rec, cnt, state = dev.find_eclipses(times, None, reference_jd=jd, kind=kind, state=True)
            if in_season:
                dur = float(rec[0, 0]["t_exit_min"] - rec[0, 0]["t_entry_min"])
                print("geostationary, jd %.1f, kind %d: %d eclipse(s), %.2f min" % (jd, kind, int(cnt[0]), dur))
                assert cnt[0] == 1 and int(rec[0, 0]["flags"]) == 0 and 55.0 < dur < 80.0
                assert int((state[0] == 2).sum()) in range(60, 75)
            else:
                assert cnt[0] == 0 and not state.any()
    # a dawn-dusk sun-synchronous member (node 90 degrees ahead of the Sun) at an equinox: beta = 82 degrees against the 64 an
    # eclipse needs at 700 km -- none, and an all-zero state row; the same orbit with its node at the Sun is eclipsed every rev
    jd = _jd(2025, 3, 20)
    sun = native.sun_position(jd)
    ra = np.degrees(np.arctan2(sun[1], sun[0]))
    mm = synth._n_from_alt(700.0, 0.001)[0]
    for node, eclipsed in (((ra + 90.0) % 360.0, False), (ra % 360.0, True)):
        sso = synth.format_tle(99003, jd, 98.19, node, 0.001, 0.0, 0.0, mm, 1e-5)
        dev = native.DeviceConstellation.from_tle_lines([sso], 0, 0)
        for kind in (0, 1):
            rec, cnt, state = dev.find_eclipses(times, None, reference_jd=jd, kind=kind, state=True)
            if eclipsed:
                assert 14 <= cnt[0] <= 16
            else:
                assert cnt[0] == 0 and not state.any()


def test_eclipse_edge_cases(native, synth, case):
    import torch
    pairs, dev, ref, off, times, res = case
    rec, cnt, state = res[0]
    # room for fewer records than there are intervals: the first ones, and the true count
    r1, c1 = dev.find_eclipses(times, off, reference_jd=ref, max_eclipses=1)
    assert np.array_equal(c1, cnt)
    has = cnt > 0
    assert r1[has, 0].tobytes() == rec[has, 0].tobytes()
    r0, c0 = dev.find_eclipses(times, off, reference_jd=ref, max_eclipses=0)
    assert np.array_equal(c0, cnt) and r0.size == 0
    # in shadow at the first / last grid time: flagged, with the grid times
    first = rec[:, 0][(cnt > 0) & ((rec[:, 0]["flags"] & native.ECLIPSE_IN_AT_START) != 0)]
    assert len(first) > 10 and (first["t_entry_min"] == times[0]).all() and (first["grid_entry"] == 0).all()
    last = np.array([rec[s, cnt[s] - 1] for s in range(dev.n) if cnt[s]])
    last = last[(last["flags"] & native.ECLIPSE_IN_AT_END) != 0]
    assert len(last) > 10 and (last["t_exit_min"] == times[-1]).all() and (last["grid_exit"] == len(times) - 1).all()
    assert ((state[:, 0] == 2).sum(), (state[:, -1] == 2).sum()) == (len(first), len(last))
    # argument checks
    L = native.lib()
    t = np.ascontiguousarray(times[:8])
    c8 = np.zeros(dev.n, dtype=np.uint32)
    call = lambda tt, jd, kind: L.azh_find_eclipses_host(dev._h, tt.ctypes.data, len(tt), off.ctypes.data, jd, kind, None, 0,  # noqa: E731
                                                         c8.ctypes.data, None)
    assert call(t, ref, 0) == 0
    for bad_t in (np.array([0.0, 1.0, 1.0]), np.array([2.0, 1.0]), np.array([0.0, np.nan, 2.0])):
        assert call(bad_t, ref, 0) == VALUE
    for bad_jd in (0.0, -1.0, float("nan")):
        assert call(t, bad_jd, 0) == VALUE
    assert call(t, ref, 2) == VALUE and call(t, ref, -1) == VALUE
    assert L.azh_find_eclipses_host(dev._h, t.ctypes.data, len(t), off.ctypes.data, ref, 0, None, 4, c8.ctypes.data, None) == NULL
    assert L.azh_find_eclipses_host(dev._h, t.ctypes.data, len(t), off.ctypes.data, ref, 0, None, 0, None, None) == NULL
    c8[:] = 7
    assert call(t[:0], ref, 0) == 0 and not c8.any()  # no grid point: zero counts
    # _host and _device (torch buffers, a foreign stream) give identical bytes, state included
    for kind in (0, 1):
        rec, cnt, state = res[kind]
        mp = rec.shape[1]
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            d_out = torch.zeros(dev.n * mp * 32, dtype=torch.uint8, device="cuda")
            d_n = torch.zeros(dev.n, dtype=torch.int32, device="cuda")
            d_state = torch.full((dev.n, len(times)), 77, dtype=torch.uint8, device="cuda")
        stream.synchronize()
        dev.find_eclipses_device(times, off, d_out.data_ptr(), mp, d_n.data_ptr(), reference_jd=ref, kind=kind,
                                 d_state=d_state.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        assert np.array_equal(d_n.cpu().numpy().astype(np.uint32), cnt)
        got = d_out.cpu().numpy().view(native.ECLIPSE_DTYPE).reshape(dev.n, mp)
        for s in range(dev.n):
            k = min(int(cnt[s]), mp)
            assert got[s, :k].tobytes() == rec[s, :k].tobytes()
        assert np.array_equal(d_state.cpu().numpy(), state)
    # a satellite whose propagation fails mid-grid (perigee inside the Earth near some perigee passages), on a date that puts
    # the grid point before its first failure into the umbra: that interval is cut by the error
    bad = synth.format_tle(99100, synth.START_JD, 63.4, 10.0, 0.49, 270.0, 0.0, 6.1, 0.01)
    one = native.DeviceConstellation.from_tle_lines([bad], 0, 0)
    e = np.zeros((1, len(times)), dtype=np.uint8)
    p = np.empty((1, len(times), 3))
    one.propagate_host(times, None, pos=p, err=e, mode=native.OUT_TEME, layout=native.SAT_MAJOR)
    fail = int(np.flatnonzero(e[0])[0])
    assert 10 < fail < len(times) - 10 and not e[0, :fail].any()
    dates = [synth.START_JD + k for k in range(0, 366, 3)]
    dates = [jd for jd in dates if native.shadow_state(p[0, fail - 1], native.sun_position(jd + times[fail - 1] / 1440.0))[0] == 2]
    assert dates
    rr, cc, ss = one.find_eclipses(times, None, reference_jd=dates[0], max_eclipses=64, state=True)
    cut = [g for g in rr[0, :int(cc[0])] if g["grid_exit"] == fail - 1]
    assert len(cut) == 1 and int(cut[0]["flags"]) & native.ECLIPSE_CUT_BY_ERROR
    assert cut[0]["t_exit_min"] == times[fail - 1]
    assert np.array_equal(ss[0] == 255, e[0] != 0) and ss[0, fail] == 255 and ss[0, fail - 1] == 2


def test_several_row_windows(native, synth):
    """13,478 x 1,440: the scratch takes two row windows; the rows of the second one against a handle that holds only them."""
    pairs = synth.synth_catalog(13478, 0)
    dev = native.DeviceConstellation.from_tle_lines(pairs, native.WGS72, 0)
    times = np.arange(1440.0)
    ref = synth.START_JD
    off = (ref - dev.epochs) * 1440.0
    rec, cnt, state = dev.find_eclipses(times, off, reference_jd=ref, kind=1, max_eclipses=20, state=True)
    assert int(cnt.max()) <= 20 and int(cnt.sum()) > 150_000
    rows = np.arange(7000, 13478, dtype=np.uint32)  # (a window holds 7,608 rows of this grid)
    part = dev.subset(rows)
    r2, c2, s2 = part.find_eclipses(times, off[rows], reference_jd=ref, kind=1, max_eclipses=20, state=True)
    assert np.array_equal(c2, cnt[rows]) and np.array_equal(s2, state[rows])
    for f in ("flags", "grid_entry", "grid_exit"):
        assert np.array_equal(r2[f], rec[rows][f])
    assert np.abs(r2["t_entry_min"] - rec[rows]["t_entry_min"]).max() <= 1e-9
    assert np.abs(r2["t_exit_min"] - rec[rows]["t_exit_min"]).max() <= 1e-9


def test_python_end_to_end(native, synth):
    import astroz_amd
    pairs = synth.synth_catalog(n_near=40, seed=77)
    text = synth.pairs_to_text(pairs)
    const = astroz_amd.Constellation(text)
    when = datetime.fromtimestamp((synth.START_JD - 2440587.5) * 86400.0, tz=timezone.utc)
    start = astroz_amd._jd_of(when)
    times = np.arange(0.0, 1440.0)
    ec = astroz_amd.eclipses(text, times, start_time=when)
    assert ec.dtype == astroz_amd.ECLIPSE_DTYPE and ec.dtype.names == ("sat", "entry", "exit", "flags")
    assert len(ec) > 400
    key = ec["sat"].astype(np.float64) * 1e6 + ec["entry"]
    assert (np.diff(key) > 0).all()  # sorted by (sat, entry)
    assert (ec["entry"] <= ec["exit"]).all()
    # the same rows from the native call
    rec, cnt = const._dev.find_eclipses(times, (start - const._dev.epochs) * 1440.0, reference_jd=start, max_eclipses=64)
    flat = np.concatenate([rec[s, :cnt[s]] for s in range(len(cnt))])
    assert len(ec) == int(cnt.sum())
    assert np.array_equal(ec["entry"], flat["t_entry_min"]) and np.array_equal(ec["exit"], flat["t_exit_min"])
    assert np.array_equal(ec["flags"], flat["flags"]) and np.array_equal(ec["sat"], np.repeat(np.arange(len(cnt)), cnt))
    # with the state matrix; any shadow starts earlier and ends later than the umbra
    pen, state = astroz_amd.eclipses(const, times, kind="penumbra", start_time=when, state=True)
    assert state.shape == (const.num_satellites, len(times)) and state.dtype == np.uint8 and set(np.unique(state)) <= {0, 1, 2}
    assert len(pen) >= len(ec)
    assert np.array_equal(astroz_amd.eclipses(const, times, start_time=when, state=True)[1], state)
    # overflow: more intervals per satellite than the wrapper's first guess of room (three days)
    long_t = np.arange(0.0, 3 * 1440.0)
    ec3 = astroz_amd.eclipses(const, long_t, start_time=when)
    rec3, cnt3 = const._dev.find_eclipses(long_t, (start - const._dev.epochs) * 1440.0, reference_jd=start, max_eclipses=256)
    assert int(cnt3.max()) > 32 and len(ec3) == int(cnt3.sum())
    assert np.array_equal(ec3["entry"], np.concatenate([rec3[s, :cnt3[s]]["t_entry_min"] for s in range(len(cnt3))]))
    with pytest.raises(ValueError):
        astroz_amd.eclipses(const, times, kind="antumbra", start_time=when)
    # the Sun the finder used
    sun = astroz_amd.sun_position(start + times / 1440.0)
    assert sun.shape == (len(times), 3) and np.abs(np.linalg.norm(numpy_sun(start) - sun[0])) < 1e-3
