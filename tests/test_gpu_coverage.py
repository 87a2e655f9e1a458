"""Ground coverage (azh_coverage_*, astroz_amd.coverage) on the GPU: the counts against the rasterised records of the station
pass finder (exactly), against elevations computed in numpy from the oracle's Earth-fixed positions, every statistic against
its definition, partial time chunks and point blocks, several row windows, a member that fails inside the grid, the device
variant, argument checks, the handle's observer, and the public call end to end."""
from datetime import datetime, timezone

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = 1.0 / 298.257223563
E2 = 2.0 * F - F * F
A = 6378.137
OBS = (47.3, 8.5, 0.4)
# test_gpu_station_passes' stations: the poles, the equator, a southern site, lon +-180 and a 4-km-high site; masks 0 to 30 degrees
STATIONS = np.array([OBS, (89.9, 0.0, 0.0), (-89.9, 45.0, 0.1), (0.0, 0.0, 0.0), (0.0, 100.0, 0.0), (-33.9, 151.2, 0.05),
                     (12.0, 180.0, 0.0), (-61.0, -180.0, 3.0), (35.0, 60.0, 4.0), (60.0, -150.0, 0.2)])
MASKS = np.array([10.0, 0.0, 5.0, 10.0, 30.0, 5.0, 10.0, 0.0, 10.0, 30.0])
VALUE, NULL = -20, -101


@pytest.fixture(scope="module")
def synth():
    from astroz_amd import synth as s
    return s


def rasterise(rec, cnt, n_times):
    """The counts the pass records (S, n, max_passes) stand for: 1 on [grid_rise, grid_set] of every record."""
    assert int(cnt.max(initial=0)) <= rec.shape[2]
    out = np.zeros((rec.shape[0], n_times + 1), dtype=np.int64)
    for st in range(rec.shape[0]):
        r = rec[st][np.arange(rec.shape[2]) < cnt[st][:, None]]
        np.add.at(out[st], r["grid_rise"], 1)
        np.add.at(out[st], r["grid_set"].astype(np.int64) + 1, -1)
    return np.cumsum(out, axis=1)[:, :n_times].astype(np.uint32)


@pytest.fixture(scope="module")
def case(native, synth):
    """test_gpu_station_passes' catalog (near-earth and deep-space members, one eccentric and one geostationary), one day at
    one-minute steps, its ten stations: the station finder's records, rasterised, and the coverage call's answer."""
    pairs = synth.synth_catalog(n_near=197, n_deep=3, seed=41)
    gmst = np.degrees(native.lib().coords_julian_to_gmst(synth.START_JD))
    pairs.append(synth.format_tle(99001, synth.START_JD, 63.4, 40.0, 0.25, 270.0, 10.0, 9.0, 1e-5))
    pairs.append(synth.format_tle(99002, synth.START_JD, 0.05, (gmst + OBS[1] + 10.0) % 360.0, 0.0002, 0.0, 0.0, 1.00273791, 0.0))
    dev = native.DeviceConstellation.from_tle_lines(pairs, 0, 0)
    ref = synth.START_JD
    off = (ref - dev.epochs) * 1440.0
    times = np.arange(0.0, 1440.0)
    rec, cnt = dev.find_passes_stations(times, off, STATIONS, MASKS, reference_jd=ref, max_passes=32)
    want = rasterise(rec, cnt, len(times))
    stats, counts = dev.coverage(times, off, STATIONS, MASKS, reference_jd=ref, counts=True)
    return pairs, dev, ref, off, times, want, stats, counts


def test_counts_match_station_finder(native, case):
    pairs, dev, ref, off, times, want, stats, counts = case
    assert counts.shape == (len(STATIONS), len(times)) and counts.dtype == np.uint32
    assert stats.shape == (len(STATIONS),) and stats.dtype == native.COVERAGE_DTYPE
    assert np.array_equal(counts, want)
    assert int(want.sum()) > 10_000 and int(want.max()) > 5
    # the geostationary member is up all day from the first station
    assert int(stats["min_in_view"][0]) >= 1 and int(counts[0].min()) >= 1


def enu_elevation(p, station):
    lat, lon = np.radians(station[0]), np.radians(station[1])
    n = A / np.sqrt(1.0 - E2 * np.sin(lat) ** 2)
    r0 = np.array([(n + station[2]) * np.cos(lat) * np.cos(lon), (n + station[2]) * np.cos(lat) * np.sin(lon),
                   (n * (1.0 - E2) + station[2]) * np.sin(lat)])
    e = np.array([-np.sin(lon), np.cos(lon), 0.0])
    nn = np.array([-np.sin(lat) * np.cos(lon), -np.sin(lat) * np.sin(lon), np.cos(lat)])
    u = np.array([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)])
    enu = (p - r0) @ np.stack([e, nn, u]).T
    return np.arctan2(enu[..., 2], np.hypot(enu[..., 0], enu[..., 1]))


def test_counts_against_oracle(native, orc, case):
    """Independent of the library's geometry: the oracle's ECEF positions, elevation in numpy.  A (point, satellite, time)
    whose elevation lies within 1e-8 rad of its mask is left out (the GPU and oracle positions differ by ~6e-8 km, ~1e-10 rad
    at LEO ranges): the GPU count of a cell lies between the sure cases and the sure cases plus those left out, of which
    there are at most 8 in ~2.4 million."""
    pairs, dev, ref, off, times, want, stats, counts = case
    t = times[:240]
    lat, lon = np.meshgrid([-89.5, -45.0, 0.0, 45.0, 89.5], np.linspace(-180.0, 180.0, 10), indexing="ij")
    pts = np.stack([lat.ravel(), lon.ravel(), np.linspace(0.0, 2.0, 50)], axis=1)
    mk = np.array([0.0, 5.0, 10.0, 30.0])[np.arange(50) % 4]
    cat = orc.Catalog.from_pairs(pairs, 0)
    e0, p0, _ = cat.propagate(t, off, velocities=False, mode=orc.ECEF, reference_jd=ref, threads=16)
    assert p0.shape == (dev.n, len(t), 3)
    _, got = dev.coverage(t, off, pts, mk, reference_jd=ref, counts=True)
    ok = e0 == 0
    left_out = 0
    for k in range(len(pts)):
        d = enu_elevation(p0, pts[k]) - np.radians(mk[k])
        sure = (ok & (d >= 1e-8)).sum(axis=0)
        near = (ok & (np.abs(d) < 1e-8)).sum(axis=0)
        left_out += int(near.sum())
        assert (got[k] >= sure).all() and (got[k] <= sure + near).all(), k
    print("left out: %d of %d" % (left_out, len(pts) * dev.n * len(t)))
    assert left_out <= 8
    assert int(got.sum()) > 10_000


def stats_by_definition(row, times, k):
    """One point's azh_coverage record from its counts, by the definitions of the header."""
    n = len(times)
    o = np.zeros((), dtype=[("mean_in_view", "<f8"), ("max_gap_min", "<f8"), ("n_covered", "<u4"), ("min_in_view", "<u4"),
                            ("max_in_view", "<u4"), ("n_gaps", "<u4"), ("grid_gap_start", "<u4"), ("grid_gap_end", "<u4"),
                            ("flags", "<u4"), ("reserved", "<u4")])
    if n == 0:
        return o
    cov = row >= k
    o["mean_in_view"] = float(row.astype(np.int64).sum()) / n
    o["n_covered"], o["min_in_view"], o["max_in_view"] = int(cov.sum()), int(row.min()), int(row.max())
    gaps, a = [], None
    for i in range(n):
        if not cov[i] and a is None:
            a = i
        if cov[i] and a is not None:
            gaps.append((a, i - 1))
            a = None
    if a is not None:
        gaps.append((a, n - 1))
    o["n_gaps"] = len(gaps)
    best = None
    for a, b in gaps:
        length = times[min(b + 1, n - 1)] - times[max(a - 1, 0)]
        if best is None or length > best[0]:
            best = (length, a, b)
    if best is not None:
        o["max_gap_min"], o["grid_gap_start"], o["grid_gap_end"] = best
        o["flags"] = (1 if best[1] == 0 else 0) | (2 if best[2] == n - 1 else 0)
    return o


def assert_stats(native, stats, counts, times, k):
    assert stats.dtype == native.COVERAGE_DTYPE
    for p in range(len(stats)):
        w = stats_by_definition(counts[p], times, k)
        for f in ("n_covered", "min_in_view", "max_in_view", "n_gaps", "grid_gap_start", "grid_gap_end", "flags", "reserved"):
            assert int(stats[f][p]) == int(w[f]), (p, f, stats[p], w)
        assert stats["max_gap_min"][p] == w["max_gap_min"], (p, stats[p], w)
        assert abs(stats["mean_in_view"][p] - w["mean_in_view"]) <= 1e-12 * abs(w["mean_in_view"]), (p, stats[p], w)


def test_statistics(native, case):
    pairs, dev, ref, off, times, want, stats, counts = case
    irregular = np.sort(np.unique(np.random.default_rng(5).uniform(0.0, 1440.0, 300)))
    assert len(irregular) == 300
    _, irr_counts = dev.coverage(irregular, off, STATIONS, MASKS, reference_jd=ref, counts=True)
    for k in (1, 2, 5):
        s, c = dev.coverage(times, off, STATIONS, MASKS, reference_jd=ref, min_satellites=k, counts=True)
        assert np.array_equal(c, counts)
        assert_stats(native, s, counts, times, k)
        s, c = dev.coverage(irregular, off, STATIONS, MASKS, reference_jd=ref, min_satellites=k, counts=True)
        assert np.array_equal(c, irr_counts)
        assert_stats(native, s, irr_counts, irregular, k)
        assert int(s["n_gaps"].max()) > 3
    # the longest gap open at one end only: grids that begin or end inside the longest interior gap of the day
    s = dev.coverage(times, off, STATIONS, MASKS, reference_jd=ref)
    p = int(np.argmax(s["max_gap_min"]))
    a, b = int(s["grid_gap_start"][p]), int(s["grid_gap_end"][p])
    assert int(s["flags"][p]) == 0 and b - a >= 8
    m = (a + b) // 2
    for sub, flag in ((times[m:b + 3], 1), (times[max(a - 2, 0):m + 1], 2)):
        s1, c1 = dev.coverage(sub, off, STATIONS[p:p + 1], MASKS[p:p + 1], reference_jd=ref, counts=True)
        assert_stats(native, s1, c1, sub, 1)
        assert int(s1["flags"][0]) == flag
    # always covered: no gaps, the gap fields are zero
    s = dev.coverage(times, off, STATIONS[:1], MASKS[:1], reference_jd=ref)
    assert int(s["n_covered"][0]) == len(times) and int(s["n_gaps"][0]) == 0
    assert s["max_gap_min"][0] == 0.0 and not (s["grid_gap_start"][0] or s["grid_gap_end"][0] or s["flags"][0])
    # never covered: one gap, open at both ends, as long as the grid
    s = dev.coverage(times, off, STATIONS, MASKS, reference_jd=ref, min_satellites=10_000)
    assert not s["n_covered"].any() and (s["n_gaps"] == 1).all() and (s["flags"] == 3).all()
    assert (s["max_gap_min"] == times[-1] - times[0]).all()
    assert not s["grid_gap_start"].any() and (s["grid_gap_end"] == len(times) - 1).all()
    assert_stats(native, s, counts, times, 10_000)
    # one grid time, and none
    for k in (1, 10_000):
        s, c = dev.coverage(times[:1], off, STATIONS, MASKS, reference_jd=ref, min_satellites=k, counts=True)
        assert np.array_equal(c, counts[:, :1])
        assert_stats(native, s, c, times[:1], k)
    assert (s["n_gaps"] == 1).all() and (s["flags"] == 3).all() and not s["max_gap_min"].any()
    s, c = dev.coverage(times[:0], off, STATIONS, MASKS, reference_jd=ref, counts=True)
    assert c.shape == (len(STATIONS), 0) and not s.view(np.uint8).any()


def test_shape_edges(native, case):
    """More points than one point block, grids that end inside a chunk of 64 times, the points cut into unequal calls."""
    pairs, dev, ref, off, times, want, stats, counts = case
    lat, lon = np.meshgrid(np.linspace(-85.0, 85.0, 15), np.linspace(-180.0, 162.0, 10), indexing="ij")
    pts = np.stack([lat.ravel(), lon.ravel(), np.linspace(0.0, 2.0, 150)], axis=1)
    mk = np.array([0.0, 5.0, 10.0, 30.0])[np.arange(150) % 4]
    rec, cnt = dev.find_passes_stations(times[:129], off, pts, mk, reference_jd=ref, max_passes=8)
    full = rasterise(rec, cnt, 129)
    for n in (1, 63, 64, 65, 129):
        t = times[:n]
        s, c = dev.coverage(t, off, pts, mk, reference_jd=ref, min_satellites=2, counts=True)
        assert c.shape == (150, n)
        assert np.array_equal(c, full[:, :n]), n  # (a grid that stops earlier sees the same states at its times)
        assert_stats(native, s, c, t, 2)
        parts = [dev.coverage(t, off, pts[lo:hi], mk[lo:hi], reference_jd=ref, min_satellites=2, counts=True)
                 for lo, hi in ((0, 50), (50, 114), (114, 150))]
        assert np.concatenate([p[0] for p in parts]).tobytes() == s.tobytes()
        assert np.concatenate([p[1] for p in parts]).tobytes() == c.tobytes()
    assert int(full.sum()) > 1000


def test_several_row_windows(native, synth):
    """Config 2 (13,478 satellites).  On 1,440 grid times the station finder's scratch (49 bytes per state) takes two row
    windows and the positions-only one of coverage (25 bytes per state: 36,000 per row, 14,913 rows in 512 MiB) a single one;
    on 2,880 and 4,320 grid times (72,000 and 108,000 bytes per row: windows of 7,456 and 4,971 rows) coverage takes two and
    three, the last one partial.  The counts of windows after the first come from rows based at the start of the scratch and
    are added to a matrix that is zeroed once per call."""
    pairs = synth.synth_catalog(13478, 0)
    dev = native.DeviceConstellation.from_tle_lines(pairs, native.WGS72, 0)
    ref = synth.START_JD
    off = (ref - dev.epochs) * 1440.0
    st, mk = STATIONS[[0, 3, 5, 8]], MASKS[[0, 3, 5, 8]]
    for n_t, step in ((1440, 1.0), (2880, 0.5), (4320, 1.0 / 3.0)):  # (one day each: no more passes than 16 per satellite)
        times = np.arange(n_t) * step
        rec, cnt = dev.find_passes_stations(times, off, st, mk, reference_jd=ref, max_passes=16)
        want = rasterise(rec, cnt, len(times))
        s, c = dev.coverage(times, off, st, mk, reference_jd=ref, min_satellites=100, counts=True)
        assert np.array_equal(c, want), n_t
        assert int(want.sum()) > 1_000_000
        assert_stats(native, s, want, times, 100)
        # the rows of the last window alone, as a catalog of their own: they see what they add to the whole
        if n_t == 4320:
            lo = 2 * 4971
            tail = native.DeviceConstellation.from_tle_lines(pairs[lo:], native.WGS72, 0)
            head = native.DeviceConstellation.from_tle_lines(pairs[:lo], native.WGS72, 0)
            _, c_tail = tail.coverage(times, off[lo:], st, mk, reference_jd=ref, counts=True)
            _, c_head = head.coverage(times, off[:lo], st, mk, reference_jd=ref, counts=True)
            assert c_tail.any() and np.array_equal(c_head + c_tail, c)
            # statistics only: the handle's own counts buffer across the windows
            assert dev.coverage(times, off, st, mk, reference_jd=ref, min_satellites=100).tobytes() == s.tobytes()


def test_failed_propagation_is_not_in_view(native, synth):
    """test_gpu_eclipse's member that decays inside the grid (error 6 near some perigee passages), seen from the point below
    its last good position: counted there, not at any grid time where its propagation failed."""
    bad = synth.format_tle(99100, synth.START_JD, 63.4, 10.0, 0.49, 270.0, 0.0, 6.1, 0.01)
    pairs = [bad] + synth.synth_catalog(n_near=20, seed=7)
    ref = synth.START_JD
    times = np.arange(1440.0)
    one = native.DeviceConstellation.from_tle_lines([bad], 0, 0)
    off1 = (ref - one.epochs) * 1440.0
    e = np.zeros((1, len(times)), dtype=np.uint8)
    p = np.empty((1, len(times), 3))
    one.propagate_host(times, off1, pos=p, err=e, mode=native.OUT_ECEF, reference_jd=ref, layout=native.SAT_MAJOR)
    fail = int(np.flatnonzero(e[0])[0])
    assert 10 < fail < len(times) - 10 and not e[0, :fail].any()
    x, y, z = p[0, fail - 1]
    below = np.array([[np.degrees(np.arctan2(z, np.hypot(x, y))), np.degrees(np.arctan2(y, x)), 0.0], OBS])
    mk = np.array([0.0, 0.0])
    rec, cnt = one.find_passes_stations(times, off1, below, mk, reference_jd=ref, max_passes=32)
    _, c = one.coverage(times, off1, below, mk, reference_jd=ref, counts=True)
    assert np.array_equal(c, rasterise(rec, cnt, len(times)))
    assert c[0, fail - 1] == 1 and not c[:, e[0] != 0].any()
    cut = [g for g in rec[0, 0, :int(cnt[0, 0])] if g["grid_set"] == fail - 1]
    assert len(cut) == 1 and int(cut[0]["flags"]) & native.PASS_CUT_BY_ERROR
    # in a catalog: that member's share is the difference to the catalog without it
    dev = native.DeviceConstellation.from_tle_lines(pairs, 0, 0)
    rest = native.DeviceConstellation.from_tle_lines(pairs[1:], 0, 0)
    _, c_all = dev.coverage(times, (ref - dev.epochs) * 1440.0, below, mk, reference_jd=ref, counts=True)
    _, c_rest = rest.coverage(times, (ref - rest.epochs) * 1440.0, below, mk, reference_jd=ref, counts=True)
    assert np.array_equal(c_all - c_rest, c) and c_rest.any()


def test_device_variant(native, case):
    import torch
    pairs, dev, ref, off, times, want, stats, counts = case
    s2, c2 = dev.coverage(times, off, STATIONS, MASKS, reference_jd=ref, min_satellites=2, counts=True)
    P, n = len(STATIONS), len(times)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d_stats = torch.full((P * native.COVERAGE_DTYPE.itemsize,), 0x5A, dtype=torch.uint8, device="cuda")
        d_only = torch.full((P * native.COVERAGE_DTYPE.itemsize,), 0x5A, dtype=torch.uint8, device="cuda")
        d_counts = torch.full((P * n,), 777, dtype=torch.int32, device="cuda")
    stream.synchronize()
    dev.coverage_device(times, off, STATIONS, MASKS, d_stats.data_ptr(), d_counts.data_ptr(), reference_jd=ref, min_satellites=2,
                        stream=stream.cuda_stream)
    dev.coverage_device(times, off, STATIONS, MASKS, d_only.data_ptr(), None, reference_jd=ref, min_satellites=2,
                        stream=stream.cuda_stream)
    stream.synchronize()
    assert d_stats.cpu().numpy().tobytes() == s2.tobytes()
    assert d_counts.cpu().numpy().tobytes() == c2.tobytes()
    assert d_only.cpu().numpy().tobytes() == s2.tobytes()
    # statistics alone from the host variant
    assert dev.coverage(times, off, STATIONS, MASKS, reference_jd=ref, min_satellites=2).tobytes() == s2.tobytes()


def test_argument_checks(native, case):
    pairs, dev, ref, off, times, want, stats, counts = case
    L = native.lib()
    h = dev._h
    t = np.ascontiguousarray(times)
    o = np.ascontiguousarray(off)
    isz = native.COVERAGE_DTYPE.itemsize

    def call(pt, mk, n_pt, tt=t, k=1, stats_p=None, counts_p=None):
        st_a = np.full(max(1, n_pt) * isz, 0x5A, dtype=np.uint8)
        cnt_a = np.full(max(1, n_pt) * max(1, len(t)), 777, dtype=np.uint32)
        pt = np.ascontiguousarray(pt, dtype=np.float64)
        mk = np.ascontiguousarray(mk, dtype=np.float64)
        rc = L.azh_coverage_host(h, tt.ctypes.data if tt is not None else None, 0 if tt is None else len(tt), o.ctypes.data, ref,
                                 pt.ctypes.data, mk.ctypes.data, n_pt, k, st_a.ctypes.data if stats_p is None else stats_p,
                                 cnt_a.ctypes.data if counts_p is None else counts_p)
        return rc, (st_a == 0x5A).all() and (cnt_a == 777).all()

    good = STATIONS[:2]
    assert call(good, MASKS[:2], 2) == (0, False)
    for bad in ((90.5, 0.0, 0.0), (-91.0, 0.0, 0.0), (np.nan, 0.0, 0.0), (0.0, np.nan, 0.0), (0.0, 0.0, np.inf)):
        assert call([OBS, bad], MASKS[:2], 2) == (VALUE, True), bad  # nothing launched, nothing written
    for bad_mask in ((10.0, np.nan), (np.inf, 0.0)):
        assert call(good, bad_mask, 2) == (VALUE, True)
    assert call(good, MASKS[:2], 2, tt=np.array([0.0, 1.0, 1.0])) == (VALUE, True)
    assert call(good, MASKS[:2], 2, tt=np.array([0.0, 2.0, 1.0])) == (VALUE, True)
    assert call(good, MASKS[:2], 2, tt=np.array([0.0, np.nan, 1.0])) == (VALUE, True)
    assert call(good, MASKS[:2], 2, k=0) == (VALUE, True)
    # n_points x n_times overflows: refused before the point and time arrays are read
    assert L.azh_coverage_host(h, t.ctypes.data, 1 << 40, None, ref, STATIONS.ctypes.data, MASKS.ctypes.data, 1 << 30,
                               1, np.zeros(isz, dtype=np.uint8).ctypes.data, None) == VALUE
    assert L.azh_coverage_device(h, t.ctypes.data, 1 << 40, None, ref, STATIONS.ctypes.data, MASKS.ctypes.data, 1 << 30,
                                 1, np.zeros(isz, dtype=np.uint8).ctypes.data, None, None) == VALUE
    # more (point block, time chunk) workgroups than one launch holds: refused before the point array is read
    assert L.azh_coverage_host(h, t.ctypes.data, len(t), None, ref, STATIONS.ctypes.data, MASKS.ctypes.data, 1 << 28, 1,
                               np.zeros(isz, dtype=np.uint8).ctypes.data, None) == VALUE
    # NULLs
    rc, untouched = call(good, MASKS[:2], 2, tt=None)  # (no times, no pointer: valid, zeroed statistics, no counts)
    assert rc == 0 and not untouched
    zero = np.zeros(2 * isz, dtype=np.uint8)
    for args in ((None, MASKS.ctypes.data), (STATIONS.ctypes.data, None)):
        assert L.azh_coverage_host(h, t.ctypes.data, len(t), None, ref, *args, 2, 1, zero.ctypes.data, None) == NULL
        assert L.azh_coverage_device(h, t.ctypes.data, len(t), None, ref, *args, 2, 1, zero.ctypes.data, None, None) == NULL
    assert call(good, MASKS[:2], 2, stats_p=0) == (NULL, True)
    assert L.azh_coverage_host(h, None, 5, None, ref, STATIONS.ctypes.data, MASKS.ctypes.data, 2, 1, zero.ctypes.data, None) == NULL
    assert L.azh_coverage_device(h, t.ctypes.data, len(t), None, ref, STATIONS.ctypes.data, MASKS.ctypes.data, 2, 1, None, None,
                                 None) == NULL
    assert call(good, MASKS[:2], 2, counts_p=0)[0] == 0  # (no counts asked for)
    # no points: OK, nothing written, whatever the pointers
    assert call(good, MASKS[:2], 0) == (0, True)
    assert L.azh_coverage_host(h, t.ctypes.data, len(t), None, ref, None, None, 0, 1, None, None) == 0
    # the wrapper: wrong lengths, min_satellites
    with pytest.raises(ValueError):
        dev.coverage(times, off, STATIONS[:3], MASKS[:2], reference_jd=ref)
    with pytest.raises(ValueError):
        dev.coverage(times, off, np.zeros(7), 10.0, reference_jd=ref)
    for k in (0, -1, 1.5):
        with pytest.raises(ValueError):
            dev.coverage(times, off, STATIONS, MASKS, reference_jd=ref, min_satellites=k)
    for short in (off[:-1], off[:0]):
        with pytest.raises(ValueError):
            dev.coverage(times, short, STATIONS, MASKS, reference_jd=ref)
        with pytest.raises(ValueError):
            dev.coverage_device(times, short, STATIONS, MASKS, 0, None, reference_jd=ref)
    # n_times 0: statistics zeroed, counts untouched
    st_a = np.full(2 * isz, 0x5A, dtype=np.uint8)
    cnt_a = np.full(8, 777, dtype=np.uint32)
    assert L.azh_coverage_host(h, None, 0, o.ctypes.data, ref, good.ctypes.data, MASKS.ctypes.data, 2, 1, st_a.ctypes.data,
                               cnt_a.ctypes.data) == 0
    assert not st_a.any() and (cnt_a == 777).all()


def test_handle_observer_untouched(native, case):
    pairs, dev, ref, off, times, want, stats, counts = case
    t = times[:240]
    dev.set_observer(-20.0, 30.0, 1.0)
    before = np.empty((dev.n, len(t), 3))
    dev.propagate_host(t, off, pos=before, mode=native.OUT_TOPOCENTRIC, reference_jd=ref, layout=native.SAT_MAJOR)
    s, c = dev.coverage(times, off, STATIONS, MASKS, reference_jd=ref, counts=True)
    assert np.array_equal(c, counts) and s.tobytes() == stats.tobytes()
    after = np.empty_like(before)
    dev.propagate_host(t, off, pos=after, mode=native.OUT_TOPOCENTRIC, reference_jd=ref, layout=native.SAT_MAJOR)
    assert after.tobytes() == before.tobytes()
    # a handle that never had an observer: coverage works, and topocentric output still asks for one
    fresh = native.DeviceConstellation.from_tle_lines(pairs, 0, 0)
    s2, c2 = fresh.coverage(times, off, STATIONS, MASKS, reference_jd=ref, counts=True)
    assert np.array_equal(c2, counts) and s2.tobytes() == stats.tobytes()
    with pytest.raises(native.NativeError):
        fresh.propagate_host(t, off, pos=np.empty((fresh.n, len(t), 3)), mode=native.OUT_TOPOCENTRIC, reference_jd=ref,
                             layout=native.SAT_MAJOR)
    # the pass finders after a positions-only window in the shared scratch
    rec, cnt = fresh.find_passes_stations(times, off, STATIONS, MASKS, reference_jd=ref, max_passes=32)
    assert np.array_equal(rasterise(rec, cnt, len(times)), counts)


def test_coverage_end_to_end(native, synth, monkeypatch):
    import astroz_amd
    pairs = synth.synth_catalog(n_near=60, seed=78)
    const = astroz_amd.Constellation(synth.pairs_to_text(pairs))
    when = datetime.fromtimestamp((synth.START_JD - 2440587.5) * 86400.0, tz=timezone.utc)
    times = np.arange(0.0, 1440.0)
    pts = astroz_amd.grid_points(30)
    assert pts.shape == (6 * 12, 3)
    k = 2
    cov, counts = astroz_amd.coverage(const, times, pts, min_elevation=10.0, min_satellites=k, start_time=when, counts=True)
    assert cov.dtype == astroz_amd.COVERAGE_DTYPE and cov.shape == (len(pts),)
    assert cov.dtype.names == ("covered_fraction", "mean_in_view", "min_in_view", "max_in_view", "n_gaps", "max_gap", "gap_start",
                               "gap_end", "flags")
    assert counts.shape == (len(pts), len(times)) and counts.dtype == np.uint32
    assert np.array_equal(cov["covered_fraction"], (counts >= k).mean(axis=1))
    assert np.array_equal(cov["min_in_view"], counts.min(axis=1)) and np.array_equal(cov["max_in_view"], counts.max(axis=1))
    assert np.abs(cov["mean_in_view"] - counts.mean(axis=1)).max() <= 1e-12 * counts.mean(axis=1).max()
    assert 0.0 < cov["covered_fraction"].mean() < 1.0 and int(cov["n_gaps"].max()) > 3
    for p in range(len(pts)):
        w = stats_by_definition(counts[p], times, k)
        assert int(cov["n_gaps"][p]) == int(w["n_gaps"]) and cov["max_gap"][p] == w["max_gap_min"] and int(cov["flags"][p]) == int(w["flags"])
        if w["n_gaps"]:
            assert cov["gap_start"][p] == times[max(int(w["grid_gap_start"]) - 1, 0)]
            assert cov["gap_end"][p] == times[min(int(w["grid_gap_end"]) + 1, len(times) - 1)]
            assert cov["max_gap"][p] == cov["gap_end"][p] - cov["gap_start"][p]
    # without the matrix: the same rows
    assert astroz_amd.coverage(const, times, pts, min_satellites=k, start_time=when).tobytes() == cov.tobytes()
    # five of the points against the rasterised passes of station_passes (a pass holds the grid times in [rise, set])
    five = [3, 17, 30, 44, 71]
    ps = astroz_amd.station_passes(const, times, [tuple(pts[i]) for i in five], min_elevation=10.0, start_time=when)
    for j, i in enumerate(five):
        mine = ps[ps["station"] == j]
        up = ((times[None, :] >= mine["rise"][:, None]) & (times[None, :] <= mine["set"][:, None])).sum(axis=0)
        assert np.array_equal(up, counts[i]), i
    # the points split over several calls by the byte budget: identical
    monkeypatch.setattr(astroz_amd, "_COVERAGE_CALL_BYTES", 7 * 4 * len(times))
    calls = []
    real = type(const._dev).coverage
    monkeypatch.setattr(type(const._dev), "coverage", lambda self, *a, **kw: calls.append(len(a[2])) or real(self, *a, **kw))
    cov2, counts2 = astroz_amd.coverage(const, times, pts, min_elevation=10.0, min_satellites=k, start_time=when, counts=True)
    assert calls == [7] * 10 + [2]
    assert cov2.tobytes() == cov.tobytes() and counts2.tobytes() == counts.tobytes()
    # a per-point mask: a lower mask sees no less; no points
    masks = np.where(np.arange(len(pts)) % 2 == 0, 0.0, 10.0)
    _, cm = astroz_amd.coverage(const, times, pts, min_elevation=masks, start_time=when, counts=True)
    assert np.array_equal(cm[1::2], counts[1::2]) and (cm[0::2] >= counts[0::2]).all() and (cm[0::2] > counts[0::2]).any()
    assert len(astroz_amd.coverage(const, times, [], start_time=when)) == 0
