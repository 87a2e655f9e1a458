"""Passes over several ground stations in one call (azh_find_passes_stations_*, astroz_amd.station_passes) on the GPU: every
station's slice against the single-station finder at the same mask, against an independent one-second scan of the oracle,
more stations than one group, several row windows, truncation, the device variant, the handle's observer, argument checks."""
from datetime import datetime, timezone

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = 1.0 / 298.257223563
E2 = 2.0 * F - F * F
A = 6378.137
OBS = (47.3, 8.5, 0.4)
# the poles, the equator, a southern site, lon +-180 and a 4-km-high site; masks 0, 5, 10 and 30 degrees
STATIONS = np.array([OBS, (89.9, 0.0, 0.0), (-89.9, 45.0, 0.1), (0.0, 0.0, 0.0), (0.0, 100.0, 0.0), (-33.9, 151.2, 0.05),
                     (12.0, 180.0, 0.0), (-61.0, -180.0, 3.0), (35.0, 60.0, 4.0), (60.0, -150.0, 0.2)])
MASKS = np.array([10.0, 0.0, 5.0, 10.0, 30.0, 5.0, 10.0, 0.0, 10.0, 30.0])
VALUE, NULL = -20, -101


@pytest.fixture(scope="module")
def synth():
    from astroz_amd import synth as s
    return s


@pytest.fixture(scope="module")
def case(native, synth):
    """test_gpu_topocentric's pass catalog: near-earth and deep-space members, one eccentric and one geostationary, one day
    at one-minute steps."""
    pairs = synth.synth_catalog(n_near=197, n_deep=3, seed=41)
    gmst = np.degrees(native.lib().coords_julian_to_gmst(synth.START_JD))
    pairs.append(synth.format_tle(99001, synth.START_JD, 63.4, 40.0, 0.25, 270.0, 10.0, 9.0, 1e-5))
    pairs.append(synth.format_tle(99002, synth.START_JD, 0.05, (gmst + OBS[1] + 10.0) % 360.0, 0.0002, 0.0, 0.0, 1.00273791, 0.0))
    dev = native.DeviceConstellation.from_tle_lines(pairs, 0, 0)
    ref = synth.START_JD
    off = (ref - dev.epochs) * 1440.0
    times = np.arange(0.0, 1440.0)
    rec, cnt = dev.find_passes_stations(times, off, STATIONS, MASKS, reference_jd=ref, max_passes=32)
    return pairs, dev, ref, off, times, rec, cnt


def single(dev, times, off, ref, station, mask, max_passes):
    dev.set_observer(*station)
    return dev.find_passes(times, off, reference_jd=ref, min_elevation_deg=float(mask), max_passes=max_passes)


def assert_matches(got, got_cnt, want, want_cnt):
    """One station's records against the single-station finder's: same counts, flags and grid indices; times within 1e-8
    min (1e-6 for the culmination of passes longer than an hour); elevations and azimuths (mod 2 pi) within 1e-10 rad."""
    assert np.array_equal(got_cnt, want_cnt)
    k = np.minimum(want_cnt, want.shape[1])
    sel = np.arange(want.shape[1])[None, :] < k[:, None]
    g, w = got[:, :want.shape[1]][sel], want[sel]
    for f in ("flags", "grid_rise", "grid_culm", "grid_set"):
        assert np.array_equal(g[f], w[f]), f
    assert np.abs(g["t_rise_min"] - w["t_rise_min"]).max(initial=0.0) <= 1e-8
    assert np.abs(g["t_set_min"] - w["t_set_min"]).max(initial=0.0) <= 1e-8
    long_pass = (w["t_set_min"] - w["t_rise_min"]) >= 60.0
    assert (np.abs(g["t_culm_min"] - w["t_culm_min"]) <= np.where(long_pass, 1e-6, 1e-8)).all()
    assert np.abs(g["max_elevation_rad"] - w["max_elevation_rad"]).max(initial=0.0) <= 1e-10
    for f in ("rise_azimuth_rad", "set_azimuth_rad"):
        d = (g[f] - w[f] + np.pi) % (2 * np.pi) - np.pi
        assert np.abs(d).max(initial=0.0) <= 1e-10, f
    return int(sel.sum())


def stored(cnt, max_passes):
    """The record slots a call wrote (the rest of its output is left as it was)."""
    return np.arange(max_passes) < np.minimum(cnt, max_passes)[..., None]


def test_each_station_matches_single_station_finder(native, case):
    pairs, dev, ref, off, times, rec, cnt = case
    assert rec.shape == (len(STATIONS), dev.n, 32) and cnt.shape == (len(STATIONS), dev.n)
    total = 0
    for st in range(len(STATIONS)):
        w, wc = single(dev, times, off, ref, STATIONS[st], MASKS[st], 32)
        total += assert_matches(rec[st], cnt[st], w, wc)
    assert total > 1000 and int(cnt.max()) <= 32
    # the geostationary member from the first station: up all day
    assert cnt[0, -1] == 1 and int(rec[0, -1, 0]["flags"]) == native.PASS_UP_AT_START | native.PASS_UP_AT_END
    assert (rec["flags"] & native.PASS_UP_AT_START).any() and (rec["flags"] & native.PASS_UP_AT_END).any()


def enu_elevation(p, station):
    lat, lon = np.radians(station[0]), np.radians(station[1])
    n = A / np.sqrt(1.0 - E2 * np.sin(lat) ** 2)
    r0 = np.array([(n + station[2]) * np.cos(lat) * np.cos(lon), (n + station[2]) * np.cos(lat) * np.sin(lon),
                   (n * (1.0 - E2) + station[2]) * np.sin(lat)])
    e = np.array([-np.sin(lon), np.cos(lon), 0.0])
    nn = np.array([-np.sin(lat) * np.cos(lon), -np.sin(lat) * np.sin(lon), np.cos(lat)])
    u = np.array([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)])
    enu = (p - r0) @ np.stack([e, nn, u]).T
    return np.arctan2(enu[:, 2], np.hypot(enu[:, 0], enu[:, 1])), enu


def top_of(enu3):
    """Highest elevation between three samples a second apart: the east-north-up components (smooth, unlike the elevation
    near the zenith) on parabolas through them, sampled every millisecond; (offset in samples, elevation)."""
    u = np.linspace(-1.0, 1.0, 2001)[:, None]
    x = enu3[1] + 0.5 * (enu3[2] - enu3[0]) * u + 0.5 * (enu3[2] - 2.0 * enu3[1] + enu3[0]) * u * u
    el = np.arctan2(x[:, 2], np.hypot(x[:, 0], x[:, 1]))
    j = int(np.argmax(el))
    return float(u[j, 0]), float(el[j])


def test_against_one_second_scan(native, orc, case):
    """test_passes_against_one_second_scan's method for three of the stations: the oracle's ECEF track every second."""
    pairs, dev, ref, off, times, rec, cnt = case
    picks = (0, 1, 5)
    fine = np.arange(0.0, times[-1] * 60.0 + 0.5) / 60.0
    matched = 0
    for lo in range(0, dev.n, 25):
        hi = min(dev.n, lo + 25)
        sub = orc.Catalog.from_pairs(pairs[lo:hi], 0)
        e0, p0, _ = sub.propagate(fine, off[lo:hi], velocities=False, mode=orc.ECEF, reference_jd=ref, threads=16)
        for st in picks:
            min_el = np.radians(MASKS[st])
            for s in range(lo, hi):
                el, enu = enu_elevation(p0[s - lo], STATIONS[st])
                up = (e0[s - lo] == 0) & (el >= min_el)
                d = np.diff(up.astype(np.int8))
                starts, ends = list(np.flatnonzero(d == 1) + 1), list(np.flatnonzero(d == -1))
                if up[0]:
                    starts.insert(0, 0)
                if up[-1]:
                    ends.append(len(up) - 1)
                truth = []
                for a, b in zip(starts, ends):
                    tr = fine[a] if a == 0 else fine[a - 1] + (min_el - el[a - 1]) / (el[a] - el[a - 1]) / 60.0
                    ts = fine[b] if b == len(up) - 1 else fine[b] + (el[b] - min_el) / (el[b] - el[b + 1]) / 60.0
                    k = a + int(np.argmax(el[a:b + 1]))
                    tk, ek = fine[k], el[k]
                    if a < k < b:
                        u, ek = top_of(enu[k - 1:k + 2])
                        tk += u / 60.0
                    truth.append((tr, tk, ts, ek))
                got = rec[st, s, :min(int(cnt[st, s]), rec.shape[2])]
                for g in got:
                    m = [t for t in truth if t[0] - 1.0 / 60 <= g["t_culm_min"] <= t[2] + 1.0 / 60]
                    assert len(m) == 1, (st, s, g)
                    tr, tc, ts, emax = m[0]
                    assert abs(g["t_rise_min"] - tr) * 60.0 <= 2.0, (st, s, g["t_rise_min"], tr)
                    assert abs(g["t_set_min"] - ts) * 60.0 <= 2.0, (st, s, g["t_set_min"], ts)
                    assert abs(g["max_elevation_rad"] - emax) <= 1e-4, (st, s, g, emax)
                    matched += 1
                for t in truth:  # every pass found
                    if t[3] >= min_el + np.radians(0.5):
                        assert any(g["t_rise_min"] <= t[1] <= g["t_set_min"] for g in got), (st, s, t)
    assert matched == int(cnt[list(picks)].sum()) and matched > 300


def test_more_stations_than_one_group(native, case):
    pairs, dev, ref, off, times, rec, cnt = case
    lat, lon = np.meshgrid(np.linspace(-85.0, 85.0, 15), np.linspace(-180.0, 162.0, 10), indexing="ij")
    st = np.stack([lat.ravel(), lon.ravel(), np.linspace(0.0, 2.0, 150)], axis=1)
    mk = np.array([0.0, 5.0, 10.0, 30.0])[np.arange(150) % 4]
    big, big_cnt = dev.find_passes_stations(times, off, st, mk, reference_jd=ref, max_passes=24)
    assert big.shape == (150, dev.n, 24) and int(big_cnt.max()) <= 24
    # the same stations asked in calls of at most one group, cut elsewhere
    for lo, hi in ((0, 50), (50, 114), (114, 150)):
        r, c = dev.find_passes_stations(times, off, st[lo:hi], mk[lo:hi], reference_jd=ref, max_passes=24)
        assert np.array_equal(c, big_cnt[lo:hi])
        assert r[stored(c, 24)].tobytes() == big[lo:hi][stored(c, 24)].tobytes()
    for k in (0, 63, 64, 77, 128, 149):
        w, wc = single(dev, times, off, ref, st[k], mk[k], 24)
        assert_matches(big[k], big_cnt[k], w, wc)


def test_several_row_windows(native, synth):
    """Config 2 (13,478 x 1,440): the scratch takes two row windows."""
    pairs = synth.synth_catalog(13478, 0)
    dev = native.DeviceConstellation.from_tle_lines(pairs, native.WGS72, 0)
    times = np.arange(1440.0)
    ref = synth.START_JD
    off = (ref - dev.epochs) * 1440.0
    st, mk = STATIONS[[0, 3, 5, 8]], MASKS[[0, 3, 5, 8]]
    rec, cnt = dev.find_passes_stations(times, off, st, mk, reference_jd=ref, max_passes=16)
    checked = 0
    for k in range(len(st)):
        w, wc = single(dev, times, off, ref, st[k], mk[k], 16)
        assert int(cnt[k].sum()) == int(wc.sum())
        checked += assert_matches(rec[k], cnt[k], w, wc)
    assert checked == int(np.minimum(cnt, 16).sum()) and checked > 50_000


def test_truncation_and_device_variant(native, case):
    import torch
    pairs, dev, ref, off, times, rec, cnt = case
    r1, c1 = dev.find_passes_stations(times, off, STATIONS, MASKS, reference_jd=ref, max_passes=1)
    assert np.array_equal(c1, cnt)
    has = cnt > 0
    assert r1[has][:, 0].tobytes() == rec[has][:, 0].tobytes()
    r0, c0 = dev.find_passes_stations(times, off, STATIONS, MASKS, reference_jd=ref, max_passes=0)
    assert np.array_equal(c0, cnt) and r0.size == 0
    S, n, mp = len(STATIONS), dev.n, rec.shape[2]
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d_out = torch.zeros(S * n * mp * 64, dtype=torch.uint8, device="cuda")
        d_n = torch.zeros(S * n, dtype=torch.int32, device="cuda")
    stream.synchronize()
    dev.find_passes_stations_device(times, off, STATIONS, MASKS, d_out.data_ptr(), mp, d_n.data_ptr(), reference_jd=ref,
                                    stream=stream.cuda_stream)
    stream.synchronize()
    assert np.array_equal(d_n.cpu().numpy().astype(np.uint32).reshape(S, n), cnt)
    got = d_out.cpu().numpy().view(native.PASS_DTYPE).reshape(S, n, mp)
    k = stored(cnt, mp)
    assert got[k].tobytes() == rec[k].tobytes()


def test_handle_observer_untouched(native, synth, case):
    pairs, dev, ref, off, times, rec, cnt = case
    t = times[:240]
    dev.set_observer(-20.0, 30.0, 1.0)
    before = np.empty((dev.n, len(t), 3))
    dev.propagate_host(t, off, pos=before, mode=native.OUT_TOPOCENTRIC, reference_jd=ref, layout=native.SAT_MAJOR)
    r, c = dev.find_passes_stations(times, off, STATIONS, MASKS, reference_jd=ref, max_passes=32)
    assert np.array_equal(c, cnt)
    after = np.empty_like(before)
    dev.propagate_host(t, off, pos=after, mode=native.OUT_TOPOCENTRIC, reference_jd=ref, layout=native.SAT_MAJOR)
    assert after.tobytes() == before.tobytes()
    # a handle that never had an observer: the stations call works, and topocentric output still asks for one
    fresh = native.DeviceConstellation.from_tle_lines(pairs, 0, 0)
    r2, c2 = fresh.find_passes_stations(times, off, STATIONS, MASKS, reference_jd=ref, max_passes=32)
    assert np.array_equal(c2, cnt) and r2[stored(cnt, 32)].tobytes() == rec[stored(cnt, 32)].tobytes()
    with pytest.raises(native.NativeError):
        fresh.propagate_host(t, off, pos=np.empty((fresh.n, len(t), 3)), mode=native.OUT_TOPOCENTRIC, reference_jd=ref,
                             layout=native.SAT_MAJOR)


def test_argument_checks(native, synth, case):
    pairs, dev, ref, off, times, rec, cnt = case
    L = native.lib()
    h = dev._h
    n = dev.n
    t = np.ascontiguousarray(times)
    o = np.ascontiguousarray(off)
    out = np.zeros(2 * n * 4, dtype=native.PASS_DTYPE)

    def call(st, mk, n_st, tt=t, max_passes=4, out_p=None, cnt_p=None):
        cnt_a = np.full(max(1, n_st) * n, 777, dtype=np.uint32)
        st = np.ascontiguousarray(st, dtype=np.float64)
        mk = np.ascontiguousarray(mk, dtype=np.float64)
        rc = L.azh_find_passes_stations_host(h, tt.ctypes.data if tt is not None else None, 0 if tt is None else len(tt),
                                             o.ctypes.data, ref, st.ctypes.data, mk.ctypes.data, n_st,
                                             out.ctypes.data if out_p is None else out_p, max_passes,
                                             cnt_a.ctypes.data if cnt_p is None else cnt_p)
        return rc, cnt_a

    good = STATIONS[:2]
    assert call(good, MASKS[:2], 2)[0] == 0
    for bad in ((90.5, 0.0, 0.0), (-91.0, 0.0, 0.0), (np.nan, 0.0, 0.0), (0.0, np.nan, 0.0), (0.0, 0.0, np.inf)):
        rc, c = call([OBS, bad], MASKS[:2], 2)
        assert rc == VALUE and (c == 777).all(), bad  # nothing launched, nothing written
    for bad_mask in ((10.0, np.nan), (np.inf, 0.0)):
        assert call(good, bad_mask, 2)[0] == VALUE
    assert call(good, MASKS[:2], 2, tt=np.array([0.0, 1.0, 1.0]))[0] == VALUE
    assert call(good, MASKS[:2], 2, tt=np.array([0.0, 2.0, 1.0]))[0] == VALUE
    assert call(good, MASKS[:2], 2, max_passes=1 << 33)[0] == VALUE
    # n_stations x n_sats x max_passes overflows: refused before the station arrays are read
    one = np.zeros(n, dtype=np.uint32)
    rc = L.azh_find_passes_stations_host(h, t.ctypes.data, len(t), None, ref, STATIONS.ctypes.data, MASKS.ctypes.data, 1 << 60,
                                         out.ctypes.data, 1 << 20, one.ctypes.data)
    assert rc == VALUE
    # NULLs
    assert call(good, MASKS[:2], 2, tt=None)[0] == 0  # (no times, no pointer: valid, counts 0)
    rc = L.azh_find_passes_stations_host(h, t.ctypes.data, len(t), None, ref, None, MASKS.ctypes.data, 2, out.ctypes.data, 4,
                                         np.zeros(2 * n, dtype=np.uint32).ctypes.data)
    assert rc == NULL
    rc = L.azh_find_passes_stations_host(h, t.ctypes.data, len(t), None, ref, STATIONS.ctypes.data, None, 2, out.ctypes.data, 4,
                                         np.zeros(2 * n, dtype=np.uint32).ctypes.data)
    assert rc == NULL
    assert call(good, MASKS[:2], 2, out_p=0)[0] == NULL
    assert call(good, MASKS[:2], 2, cnt_p=0)[0] == NULL
    rc = L.azh_find_passes_stations_host(h, None, 5, None, ref, STATIONS.ctypes.data, MASKS.ctypes.data, 2, out.ctypes.data, 4,
                                         np.zeros(2 * n, dtype=np.uint32).ctypes.data)
    assert rc == NULL
    rc = L.azh_find_passes_stations_device(h, t.ctypes.data, len(t), None, ref, STATIONS.ctypes.data, MASKS.ctypes.data, 2, None, 4,
                                           None, None)
    assert rc == NULL
    # no stations: OK, nothing written
    rc, c = call(good, MASKS[:2], 0)
    assert rc == 0 and (c == 777).all()
    # wrong lengths in the wrapper
    with pytest.raises(ValueError):
        dev.find_passes_stations(times, off, STATIONS[:3], MASKS[:2], reference_jd=ref)
    with pytest.raises(ValueError):
        dev.find_passes_stations(times, off, np.zeros(7), 10.0, reference_jd=ref)
    # n_times 0 and 1
    r, c = dev.find_passes_stations(times[:0], off, STATIONS, MASKS, reference_jd=ref, max_passes=4)
    assert c.shape == (len(STATIONS), n) and not c.any()
    r, c = dev.find_passes_stations(times[:1], off, STATIONS, MASKS, reference_jd=ref, max_passes=4)
    for st in range(len(STATIONS)):
        w, wc = single(dev, times[:1], off, ref, STATIONS[st], MASKS[st], 4)
        assert_matches(r[st], c[st], w, wc)
    assert c.any() and (r["flags"][c > 0][:, 0] == 3).all()
    # an empty catalog: no handle holds one (the library refuses to build it), so the call never sees one
    with pytest.raises(native.NativeError) as e:
        dev.subset([])
    assert e.value.code == VALUE


def test_station_passes_end_to_end(native, synth):
    import astroz_amd
    pairs = synth.synth_catalog(n_near=60, seed=78)
    text = synth.pairs_to_text(pairs)
    const = astroz_amd.Constellation(text)
    when = datetime.fromtimestamp((synth.START_JD - 2440587.5) * 86400.0, tz=timezone.utc)
    times = np.arange(0.0, 1440.0)
    sts = [tuple(s) for s in STATIONS[:5]]
    ps = astroz_amd.station_passes(const, times, sts, min_elevation=10.0, start_time=when)
    assert ps.dtype == astroz_amd.STATION_PASS_DTYPE and ps.dtype.names[0] == "station"
    assert len(ps) > 50 and set(np.unique(ps["station"])) <= set(range(len(sts)))
    key = np.lexsort((ps["rise"], ps["sat"], ps["station"]))
    assert np.array_equal(key, np.arange(len(ps)))  # sorted by (station, sat, rise)
    assert (ps["max_elevation"] >= np.radians(10.0)).all()
    # equal to passes() per station (which sets the observer of its own call)
    for k, s in enumerate(sts):
        one = astroz_amd.passes(const, times, s, min_elevation=10.0, start_time=when)
        mine = ps[ps["station"] == k]
        assert len(mine) == len(one)
        for f in one.dtype.names:
            d = mine[f].astype(np.float64) - one[f]
            if f.endswith("azimuth"):
                d = (d + np.pi) % (2 * np.pi) - np.pi
            assert np.abs(d).max(initial=0.0) <= (0.0 if f in ("sat", "flags") else 1e-8), (k, f)
    # a per-station mask; the scalar is the same as its broadcast
    masks = [0.0, 5.0, 10.0, 30.0, 10.0]
    pm = astroz_amd.station_passes(const, times, sts, min_elevation=masks, start_time=when)
    ps10 = astroz_amd.station_passes(const, times, sts, min_elevation=[10.0] * 5, start_time=when)
    assert ps10.tobytes() == ps.tobytes()
    for k, m in enumerate(masks):
        one = astroz_amd.passes(const, times, sts[k], min_elevation=m, start_time=when)
        assert (pm["station"] == k).sum() == len(one)
    assert (pm["station"] == 0).sum() > (pm["station"] == 3).sum()  # (0 degrees sees more than 30)
    # overflow: more passes per satellite than the wrapper's first room (a 0-degree mask over 3 days)
    long_t = np.arange(0.0, 3 * 1440.0)
    p0 = astroz_amd.station_passes(const, long_t, sts[:2], min_elevation=0.0, start_time=when)
    for k in range(2):
        one = astroz_amd.passes(const, long_t, sts[k], min_elevation=0.0, start_time=when)
        mine = p0[p0["station"] == k]
        assert np.array_equal(mine["sat"], one["sat"]) and np.abs(mine["rise"] - one["rise"]).max() <= 1e-8
    assert np.bincount(p0[p0["station"] == 0]["sat"]).max() > 16
    # no stations
    assert len(astroz_amd.station_passes(const, times, [], start_time=when)) == 0
