"""The pass, eclipse and access finders off the one-minute, 1,440-point axis of their own modules, on a catalog of 26 rows:
(A) an irregular, a half-minute and a two-rate axis against the numpy restatements, the station finder against the single one,
and both against a one-second scan of the oracle; (B) grids of 1 .. 129 points, around the 64-point chunk of the kernels;
(C) 64 windows of one axis, each a point later than the last, so that every rise, set, entry, exit, start, end and error cut
is met in every lane of a wave -- the first and the last, where the state carried from chunk to chunk decides, included."""
import numpy as np
import pytest

from test_gpu_access import check_against_scan
from test_gpu_eclipse import numpy_sun, scan_eclipses, shadow, states, sun_table
from test_gpu_station_passes import MASKS, STATIONS, assert_matches, single
from test_gpu_topocentric import scan_passes, topo_from_ecef

pytestmark = pytest.mark.gpu

SEED = 41
ROW_BAD = 25  # the member whose propagation fails near some perigee passages (the last row)
PICKS = (0, 3, 5)  # of STATIONS / MASKS: 47 N at 10 degrees, the equator at 10, 34 S at 5
T0 = 0.0  # first minute of the axes of A and B (screened with the oracle: see grids())
ROOM = 32
AXES = ("irregular", "half_minute", "two_rate")
LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129)
WINDOWS, WINDOW = 64, 321  # C: windows A[s : s + 321], s < 64 -- 5 chunks, one live lane in the last
START, END, CUT = 1, 2, 4  # the flag bits, the same in the three record types (asserted in `case`)


@pytest.fixture(scope="module")
def synth():
    from astroz_amd import synth as s
    return s


@pytest.fixture(scope="module", autouse=True)
def kernel_route(native):
    """Handles this small would be served by the host route: the restatements are to read what the kernels wrote."""
    n0 = native.get_host_points()
    native.set_host_points(0)
    yield
    native.set_host_points(n0)


def event_pairs(synth):
    """24 synthetic near-earth rows, the eccentric member of the pass catalog and the member that fails mid-grid."""
    pairs = synth.synth_catalog(n_near=24, n_deep=0, seed=SEED)
    pairs.append(synth.format_tle(99001, synth.START_JD, 63.4, 40.0, 0.25, 270.0, 10.0, 9.0, 1e-5))
    pairs.append(synth.format_tle(99100, synth.START_JD, 63.4, 10.0, 0.49, 270.0, 0.0, 6.1, 0.01))
    return pairs


def grids(t0=T0):
    """The axes of A (minutes).  T0 is chosen so that a member is above the mask of a picked station and another in the umbra
    at the first point of each (the one-point grids of B), and so that no grid point lies within 1e-7 rad of a mask or 1e-7 km
    of a shadow boundary; the tests assert both, the latter at 1e-9."""
    rng = np.random.default_rng(3)
    steps = np.concatenate([np.full(100, 0.25), np.full(100, 1.5), np.full(100, 0.25)])
    return {"irregular": t0 + np.cumsum(rng.uniform(0.3, 1.7, 300)), "half_minute": t0 + (np.arange(600) * 0.5)[:300],
            "two_rate": t0 + np.concatenate([[0.0], np.cumsum(steps)]), "minute": t0 + np.arange(129.0)}


@pytest.fixture(scope="module")
def case(native, synth):
    assert (native.PASS_UP_AT_START, native.PASS_UP_AT_END, native.PASS_CUT_BY_ERROR) == (START, END, CUT)
    assert (native.ECLIPSE_IN_AT_START, native.ECLIPSE_IN_AT_END, native.ECLIPSE_CUT_BY_ERROR) == (START, END, CUT)
    assert (native.ACCESS_OPEN_AT_START, native.ACCESS_OPEN_AT_END, native.ACCESS_CUT_BY_ERROR) == (START, END, CUT)
    pairs = event_pairs(synth)
    dev = native.DeviceConstellation.from_tle_lines(pairs, 0, 0)
    assert dev.n == ROW_BAD + 1
    ref = synth.START_JD
    return pairs, dev, ref, (ref - dev.epochs) * 1440.0


# ---- the kernels' inputs, as propagate_host returns them ------------------------------------------------------------------

def topo_arrays(native, dev, times, off, ref, station):
    n, nt = dev.n, len(times)
    P, V = np.empty((n, nt, 3)), np.empty((n, nt, 3))
    E = np.zeros((n, nt), dtype=np.uint8)
    dev.set_observer(*station)
    dev.propagate_host(times, off, pos=P, vel=V, mode=native.OUT_TOPOCENTRIC, reference_jd=ref, layout=native.SAT_MAJOR, err=E)
    return P, V, E


def frame_arrays(native, dev, times, off, ref, mode):
    n, nt = dev.n, len(times)
    P, V = np.empty((n, nt, 3)), np.empty((n, nt, 3))
    E = np.zeros((n, nt), dtype=np.uint8)
    dev.propagate_host(times, off, pos=P, vel=V, mode=mode, reference_jd=ref, layout=native.SAT_MAJOR, err=E)
    return P, V, E


def cut(arrays, lo, hi):
    return tuple(a[:, lo:hi] for a in arrays)


# ---- records against the restatements ---------------------------------------------------------------------------------------

def assert_clear_of_mask(P, E, min_el):
    """The precondition of every pass comparison: no propagated grid point within 1e-9 rad of the mask."""
    d = np.abs(P[..., 1] - min_el)[E == 0]
    assert d.min(initial=1.0) >= 1e-9, d.min()


def assert_passes(rec, cnt, times, arrays, min_el):
    """find_passes' records of every row against scan_passes on that row of `arrays`, test_passes_match_grid_algorithm's gates:
    counts, flags and grid indices equal, times within 1e-9 min (1e-6 for the culmination of a pass of an hour or more), the
    highest elevation within 1e-10 rad, azimuths within 1e-9 rad mod 2 pi.  Returns the scans and the largest time difference."""
    P, V, E = arrays
    assert_clear_of_mask(P, E, min_el)
    assert int(cnt.max(initial=0)) <= rec.shape[1]
    wants, worst = [], 0.0
    for s in range(len(cnt)):
        want = scan_passes(times, P[s], V[s], E[s], min_el)
        assert cnt[s] == len(want), (s, int(cnt[s]), len(want))
        for k, w in enumerate(want):
            g = rec[s, k]
            for f in ("flags", "grid_rise", "grid_culm", "grid_set"):
                assert int(g[f]) == w[f], (s, k, f, g, w)
            for f in ("t_rise_min", "t_culm_min", "t_set_min"):
                tol = 1e-9 if f != "t_culm_min" or w["t_set_min"] - w["t_rise_min"] < 60.0 else 1e-6
                assert abs(float(g[f]) - w[f]) <= tol, (s, k, f, float(g[f]), w[f])
                if f != "t_culm_min":
                    worst = max(worst, abs(float(g[f]) - w[f]))
            assert abs(float(g["max_elevation_rad"]) - w["max_elevation_rad"]) <= 1e-10, (s, k, g, w)
            for f in ("rise_azimuth_rad", "set_azimuth_rad"):
                d = (float(g[f]) - w[f] + np.pi) % (2 * np.pi) - np.pi
                assert abs(d) <= 1e-9 and 0.0 <= float(g[f]) < 2 * np.pi, (s, k, f, float(g[f]), w[f])
        wants.append(want)
    return wants, worst


def assert_eclipses(rec, cnt, state, times, arrays, tab, kind):
    """find_eclipses' records and state matrix against scan_eclipses / states on `arrays`, test_eclipses_match_grid_algorithm's
    gates: the state equal wherever |f| >= 1e-9 km (everywhere: that no point is closer is the precondition), counts, flags
    and grid indices equal, times within 1e-9 min."""
    P, V, E = arrays
    want_state, fu, fp = states(P, E, tab)
    near_edge = (np.minimum(np.abs(fu), np.abs(fp)) < 1e-9) & (E == 0)
    assert not near_edge.any()
    assert state.dtype == np.uint8 and np.array_equal(state[~near_edge], want_state[~near_edge])
    assert int(cnt.max(initial=0)) <= rec.shape[1]
    wants, worst = [], 0.0
    for s in range(len(cnt)):
        want = scan_eclipses(times, P[s], V[s], E[s], tab, kind)
        assert cnt[s] == len(want), (kind, s, int(cnt[s]), len(want))
        for k, w in enumerate(want):
            g = rec[s, k]
            for f in ("flags", "grid_entry", "grid_exit"):
                assert int(g[f]) == w[f], (kind, s, k, f, g, w)
            assert int(g["reserved"]) == 0
            for f in ("t_entry_min", "t_exit_min"):
                assert abs(float(g[f]) - w[f]) <= 1e-9, (kind, s, k, f, float(g[f]), w[f])
                worst = max(worst, abs(float(g[f]) - w[f]))
        wants.append(want)
    return wants, worst


def kernel_sun(native, ref, times):
    return sun_table(native.sun_position(ref + times / 1440.0))


def run_passes(native, dev, times, off, ref, stations, masks, room=ROOM):
    """The single finder at every station against the restatement, and the station finder against the single one; returns
    the scans per station and the largest time difference against them."""
    got, got_cnt = dev.find_passes_stations(times, off, stations, masks, reference_jd=ref, max_passes=room)
    assert got.shape == (len(stations), dev.n, room)
    wants, worst = [], 0.0
    for k in range(len(stations)):
        rec, cnt = single(dev, times, off, ref, stations[k], masks[k], room)
        w, d = assert_passes(rec, cnt, times, topo_arrays(native, dev, times, off, ref, stations[k]), np.radians(masks[k]))
        assert_matches(got[k], got_cnt[k], rec, cnt)
        wants.append(w)
        worst = max(worst, d)
    return wants, worst


def run_eclipses(native, dev, times, off, ref, room=ROOM):
    arrays = frame_arrays(native, dev, times, off, ref, native.OUT_TEME)
    tab = kernel_sun(native, ref, times)
    wants, worst = [], 0.0
    for kind in (0, 1):
        rec, cnt, state = dev.find_eclipses(times, off, reference_jd=ref, kind=kind, max_eclipses=room, state=True)
        w, d = assert_eclipses(rec, cnt, state, times, arrays, tab, kind)
        wants.append(w)
        worst = max(worst, d)
    return wants, worst


def n_events(wants, n, first, last):
    """Events (starts after the first grid point, ends before the last) of the scans of all rows."""
    return sum((w[first] > 0) + (w[last] < n - 1) for row in wants for w in row)


# ---- A: irregular and non-unit axes -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("axis", AXES)
def test_axes_passes_match_grid_algorithm(native, case, axis):
    pairs, dev, ref, off = case
    times = grids()[axis]
    wants, worst = run_passes(native, dev, times, off, ref, STATIONS[list(PICKS)], MASKS[list(PICKS)])
    total = sum(len(row) for w in wants for row in w)
    events = sum(n_events(w, len(times), "grid_rise", "grid_set") for w in wants)
    print("%s: %d passes at %d stations, %d rises and sets inside the grid, max |dt| against the numpy scan %.3g min" %
          (axis, total, len(PICKS), events, worst))
    assert total >= 10 and events >= 20


@pytest.mark.parametrize("axis", AXES)
def test_axes_eclipses_match_grid_algorithm(native, case, axis):
    pairs, dev, ref, off = case
    times = grids()[axis]
    wants, worst = run_eclipses(native, dev, times, off, ref)
    for kind in (0, 1):
        total = sum(len(row) for row in wants[kind])
        events = n_events(wants[kind], len(times), "grid_entry", "grid_exit")
        print("%s, kind %d: %d intervals, %d entries and exits inside the grid" % (axis, kind, total, events))
        assert total >= 20 and events >= 40
    print("%s: max |dt| against the numpy scan %.3g min" % (axis, worst))


def second_axis(times):
    """Every second from the first grid time on, and the last grid time."""
    fine = times[0] + np.arange(0.0, np.floor((times[-1] - times[0]) * 60.0 + 1e-6) + 1.0) / 60.0
    return fine if fine[-1] >= times[-1] - 1e-9 else np.append(fine, times[-1])


def true_runs(t, inn, f, bad):
    """Maximal runs of `inn` on the axis t (minutes): (start, end, first index, last index, start cut, end cut), the crossings
    placed linearly between the bracketing samples of f; next to a failed sample a run ends on its own sample."""
    d = np.diff(inn.astype(np.int8))
    starts, ends = list(np.flatnonzero(d == 1) + 1), list(np.flatnonzero(d == -1))
    if inn[0]:
        starts.insert(0, 0)
    if inn[-1]:
        ends.append(len(inn) - 1)
    out = []
    for a, b in zip(starts, ends):
        cut_a, cut_b = a > 0 and bool(bad[a - 1]), b < len(inn) - 1 and bool(bad[b + 1])
        ta = t[a] if a == 0 or cut_a else t[a - 1] + f[a - 1] / (f[a - 1] - f[a]) * (t[a] - t[a - 1])
        tb = t[b] if b == len(inn) - 1 or cut_b else t[b] + f[b] / (f[b] - f[b + 1]) * (t[b + 1] - t[b])
        out.append((ta, tb, int(a), int(b), cut_a, cut_b))
    return out


def grid_runs(inn):
    d = np.diff(np.concatenate([[0], inn.astype(np.int8), [0]]))
    return list(zip(np.flatnonzero(d == 1).tolist(), (np.flatnonzero(d == -1) - 1).tolist()))


@pytest.mark.parametrize("axis", AXES)
def test_axes_passes_against_one_second_scan(native, orc, case, axis):
    """test_passes_against_one_second_scan's method on the three axes, for the single finder at the picked stations (the
    station finder is held to it above): every record is one true pass of the oracle's track sampled every second, its rise
    and set within 2 s of the truth (an end cut by an error: the grid time), its highest elevation within 1e-4 rad (1e-3
    above 85 degrees) where both intervals around the grid maximum are at most a minute long -- on longer ones the Hermite
    error, which grows with the fourth power of the step, is printed and not gated; the records' grid indices are the runs
    of the oracle's own up points at the grid times, so no pass that holds a grid point is missed and none is invented."""
    pairs, dev, ref, off = case
    times = grids()[axis]
    nt = len(times)
    fine = second_axis(times)
    cat = orc.Catalog.from_pairs(pairs, 0)
    e0, p0, _ = cat.propagate(fine, off, velocities=False, mode=orc.ECEF, reference_jd=ref, threads=16)
    eg, pg, _ = cat.propagate(times, off, velocities=False, mode=orc.ECEF, reference_jd=ref)
    matched, worst_t, worst_el, worst_el_long, n_long = 0, 0.0, 0.0, 0.0, 0
    for st in PICKS:
        min_el = np.radians(MASKS[st])
        rec, cnt = single(dev, times, off, ref, STATIONS[st], MASKS[st], ROOM)
        assert int(cnt.max()) <= ROOM
        for s in range(dev.n):
            el = topo_from_ecef(p0[s], None, STATIONS[st])[0][:, 1]
            el_g = topo_from_ecef(pg[s], None, STATIONS[st])[0][:, 1]
            assert np.abs(el_g - min_el)[eg[s] == 0].min() >= 1e-9
            truth = true_runs(fine, (e0[s] == 0) & (el >= min_el), el - min_el, e0[s] != 0)
            got = rec[s, :int(cnt[s])]
            assert [(int(g["grid_rise"]), int(g["grid_set"])) for g in got] == grid_runs((eg[s] == 0) & (el_g >= min_el)), (st, s)
            used = set()
            for g in got:
                m = [q for q, t in enumerate(truth) if t[0] - 1.0 / 60 <= g["t_culm_min"] <= t[1] + 1.0 / 60]
                assert len(m) == 1 and m[0] not in used, (st, s, g, m)
                used.add(m[0])
                tr, ts, a, b, cut_a, cut_b = truth[m[0]]
                i, j, k = int(g["grid_rise"]), int(g["grid_set"]), int(g["grid_culm"])
                if not (i > 0 and eg[s, i - 1]):
                    assert abs(g["t_rise_min"] - tr) * 60.0 <= 2.0, (st, s, g["t_rise_min"], tr)
                    worst_t = max(worst_t, abs(g["t_rise_min"] - tr) * 60.0)
                if not (j < nt - 1 and eg[s, j + 1]):
                    assert abs(g["t_set_min"] - ts) * 60.0 <= 2.0, (st, s, g["t_set_min"], ts)
                    worst_t = max(worst_t, abs(g["t_set_min"] - ts) * 60.0)
                kk = a + int(np.argmax(el[a:b + 1]))
                emax = el[kk]
                if a < kk < b:  # the top between the samples: parabola through the three around the sampled maximum
                    c2 = el[kk - 1] - 2 * el[kk] + el[kk + 1]
                    if c2 < 0:
                        u = 0.5 * (el[kk - 1] - el[kk + 1]) / c2
                        emax = el[kk] - 0.25 * (el[kk - 1] - el[kk + 1]) * u
                d_el = abs(g["max_elevation_rad"] - emax)
                steps = [times[q + 1] - times[q] for q in (k - 1, k) if 0 <= q < nt - 1]
                if max(steps) <= 1.0 + 1e-9:
                    assert d_el <= (1e-3 if emax > np.radians(85.0) else 1e-4), (st, s, g, emax)
                    worst_el = max(worst_el, d_el)
                else:
                    worst_el_long, n_long = max(worst_el_long, d_el), n_long + 1
                matched += 1
    print("%s: %d passes matched, max |dt| of a rise or set %.4f s, max |d el| %.3g rad on steps of at most a minute, "
          "%.3g rad on the %d passes with a longer step at the top (not gated)" % (axis, matched, worst_t, worst_el, worst_el_long, n_long))
    assert matched >= 10


@pytest.mark.parametrize("axis", AXES)
def test_axes_eclipses_against_one_second_scan(native, orc, case, axis):
    """test_eclipses_against_one_second_scan's method on the three axes: every record is one true interval of the oracle's
    track sampled every second under the numpy Sun, a refined end within 2 s of the truth or where the oracle's f is within
    1 km of zero (grazing crossings); the records' grid indices are the runs of the oracle's own points in shadow at the grid
    times (under the library's host Sun: the numpy series differs from it by up to 1e-9 of the direction, 7e-6 km in f)."""
    pairs, dev, ref, off = case
    times = grids()[axis]
    nt = len(times)
    fine = second_axis(times)
    cat = orc.Catalog.from_pairs(pairs, 0)
    e0, p0, _ = cat.propagate(fine, off, velocities=False, mode=orc.TEME, reference_jd=ref, threads=16)
    eg, pg, _ = cat.propagate(times, off, velocities=False, mode=orc.TEME, reference_jd=ref)
    x, _, fu, fp = shadow(p0, sun_table(numpy_sun(ref + fine / 1440.0)))
    xg, _, fug, fpg = shadow(pg, kernel_sun(native, ref, times))
    assert np.minimum(np.abs(fug), np.abs(fpg))[eg == 0].min() >= 1e-9
    for kind in (0, 1):
        rec, cnt = dev.find_eclipses(times, off, reference_jd=ref, kind=kind, max_eclipses=ROOM)
        assert int(cnt.max()) <= ROOM
        fk, fkg = (fp, fpg) if kind else (fu, fug)
        matched, worst, grazing = 0, 0.0, 0
        for s in range(dev.n):
            f = fk[s]
            truth = true_runs(fine, (e0[s] == 0) & (x[s] > 0) & (f < 0), f, e0[s] != 0)
            got = rec[s, :int(cnt[s])]
            assert [(int(g["grid_entry"]), int(g["grid_exit"])) for g in got] == grid_runs((eg[s] == 0) & (xg[s] > 0) & (fkg[s] < 0)), (kind, s)
            used = set()
            for g in got:
                i, j = int(g["grid_entry"]), int(g["grid_exit"])
                m = [q for q, t in enumerate(truth) if t[0] - 1.0 / 60 <= times[i] <= t[1] + 1.0 / 60]
                assert len(m) == 1 and m[0] not in used, (kind, s, g, m)
                used.add(m[0])
                ends = []
                if not (i > 0 and eg[s, i - 1]):
                    ends.append((float(g["t_entry_min"]), truth[m[0]][0]))
                if not (j < nt - 1 and eg[s, j + 1]):
                    ends.append((float(g["t_exit_min"]), truth[m[0]][1]))
                for t_rep, t_true in ends:
                    dt_s = abs(t_rep - t_true) * 60.0
                    f_there = abs(float(np.interp(t_rep, fine, f)))
                    assert dt_s <= 2.0 or f_there <= 1.0, (kind, s, g, t_true, dt_s, f_there)
                    if dt_s <= 2.0:
                        worst = max(worst, dt_s)
                    else:
                        grazing += 1
                matched += 1
        print("%s, kind %d: %d intervals matched, max |dt| of an entry or exit %.4f s, %d ends within 1 km of grazing instead" %
              (axis, kind, matched, worst, grazing))
        assert matched >= 20


# ---- B: grid lengths around the chunk size --------------------------------------------------------------------------------

@pytest.mark.parametrize("n", LENGTHS)
def test_chunk_edge_lengths(native, case, n):
    pairs, dev, ref, off = case
    stations, masks = STATIONS[list(PICKS)], MASKS[list(PICKS)]
    for axis in ("minute", "irregular"):
        times = np.ascontiguousarray(grids()[axis][:n])
        pw, _ = run_passes(native, dev, times, off, ref, stations, masks)
        ew, _ = run_eclipses(native, dev, times, off, ref)
        p_events = sum(n_events(w, n, "grid_rise", "grid_set") for w in pw)
        e_events = [n_events(w, n, "grid_entry", "grid_exit") for w in ew]
        print("%s[:%d]: %d passes with %d rises and sets inside, %d / %d intervals with %d / %d entries and exits inside" %
              (axis, n, sum(len(r) for w in pw for r in w), p_events, sum(len(r) for r in ew[0]), sum(len(r) for r in ew[1]),
               e_events[0], e_events[1]))
        if n >= 63:  # something happens inside every such prefix, for every finder
            assert p_events >= 1 and min(e_events) >= 1
        if n == 1:  # one grid point: whoever is up or in shadow has one record, open at both ends, on the grid time
            up = [(k, s) for k in range(len(stations)) for s in range(dev.n) if pw[k][s]]
            assert up
            got, got_cnt = dev.find_passes_stations(times, off, stations, masks, reference_jd=ref, max_passes=2)
            for k, s in up:
                g = got[k, s, 0]
                assert got_cnt[k, s] == 1 and int(g["flags"]) == START | END
                assert g["t_rise_min"] == times[0] and g["t_set_min"] == times[0] and g["t_culm_min"] == times[0]
                r1, c1 = single(dev, times, off, ref, stations[k], masks[k], 2)
                assert c1[s] == 1 and int(r1[s, 0]["flags"]) == START | END
                assert r1[s, 0]["t_rise_min"] == times[0] and r1[s, 0]["t_set_min"] == times[0]
            for kind in (0, 1):
                dark = [s for s in range(dev.n) if ew[kind][s]]
                assert dark
                rec, cnt = dev.find_eclipses(times, off, reference_jd=ref, kind=kind, max_eclipses=2)
                for s in dark:
                    assert cnt[s] == 1 and int(rec[s, 0]["flags"]) == START | END
                    assert rec[s, 0]["t_entry_min"] == times[0] and rec[s, 0]["t_exit_min"] == times[0]


# ---- C: every event at every lane -------------------------------------------------------------------------------------------

CATEGORIES = ("refined start", "refined end", "start cut by error", "end cut by error")


def events_of(i, j, bad, n):
    """The events of a record on grid points i .. j of an n-point row: (category, the grid point whose lane owns the event --
    the first point inside for a start, the first point outside for an end)."""
    out = []
    if i > 0:
        out.append((CATEGORIES[2] if bad[i - 1] else CATEGORIES[0], i))
    if j < n - 1:
        out.append((CATEGORIES[3] if bad[j + 1] else CATEGORIES[1], j + 1))
    return out


class Tally:
    """What a sweep met, from the restatements alone: per category the events of the whole axis that lie inside every window
    (with their brackets), and per window the lanes at which events of that category fell; the records of a window that
    continue from one chunk into the next."""

    def __init__(self):
        self.interior = dict.fromkeys(CATEGORIES, 0)
        self.interior_long = 0
        self.lanes = {c: np.zeros(64, dtype=np.int64) for c in CATEGORIES}
        self.carried = 0

    def whole_axis(self, spans, bad, n):
        for i, j in spans:
            for c, e in events_of(i, j, bad, n):
                self.interior[c] += WINDOWS <= e <= WINDOW - 1
            self.interior_long += WINDOWS - 1 <= i < j <= WINDOW - 1  # (two points or more: over a chunk edge in some window)

    def window(self, spans, bad, n):
        for i, j in spans:
            for c, e in events_of(i, j, bad, n):
                self.lanes[c][e % 64] += 1
            self.carried += i // 64 != j // 64

    def check(self, what):
        print("%s: on the whole axis, inside every window: %s, %d records of two points or more; over the %d windows: %s, "
              "%d records carried over a chunk edge" %
              (what, ", ".join("%d %s" % (self.interior[c], c) for c in CATEGORIES), self.interior_long, WINDOWS,
               ", ".join("%s at lane 0 / 63: %d / %d" % (c, self.lanes[c][0], self.lanes[c][63]) for c in CATEGORIES), self.carried))
        for c in CATEGORIES:
            assert self.interior[c] >= 1, (what, c)
            assert self.lanes[c].min() >= 1, (what, c, self.lanes[c])  # every lane, the first and the last among them
        assert self.interior_long >= 1 and self.carried >= 1


def spans(want, first, last):
    return [(w[first], w[last]) for w in want]


@pytest.fixture(scope="module")
def sweep(native, case):
    """The one-minute axis of 64 + 321 points centred on the failing member's first run of failed grid points (found as
    test_pass_edge_cases finds it), and the two stations under its last good position before the run and its first after:
    at sea level, half a degree of latitude (55 km) from the point below it.  The member is 40 km up there, so it stands some
    35 degrees high; straight overhead its azimuth would be noise, and the records of two propagations could not be held
    to each other."""
    pairs, dev, ref, off = case
    day = np.arange(0.0, 1440.0)
    p, _, e = frame_arrays(native, dev, day, off, ref, native.OUT_ECEF)
    assert not e[:ROW_BAD].any()
    f0 = int(np.flatnonzero(e[ROW_BAD])[0])
    f1 = f0 + int(np.flatnonzero(e[ROW_BAD, f0:] == 0)[0]) - 1  # the run is grid points f0 .. f1: the member recovers
    start = (f0 + f1 + 1) // 2 - (WINDOWS + WINDOW) // 2
    axis = start + np.arange(0.0, WINDOWS + WINDOW)
    g0, g1 = f0 - 1 - start, f1 + 1 - start  # on the axis: the last good point before the run, the first after
    assert WINDOWS <= g0 and g1 + 1 <= WINDOW - 1 and start >= 0 and start + len(axis) <= len(day)
    under = []
    for g in (g0, g1):
        lla = np.zeros(3)
        x = np.ascontiguousarray(p[ROW_BAD, start + g])
        native.lib().coords_ecef_to_geodetic(x.ctypes.data, lla.ctypes.data)
        under.append((lla[0] + 0.5, lla[1], 0.0))
    return axis, g0, g1, under


def test_every_lane_passes(native, case, sweep):
    """find_passes and find_passes_stations: two ordinary stations and the two under the failing member, which see a pass
    whose set and one whose rise is cut by its error."""
    pairs, dev, ref, off = case
    axis, g0, g1, under = sweep
    stations = np.array([STATIONS[0], STATIONS[5]] + under)
    masks = np.array([MASKS[0], MASKS[5], 10.0, 10.0])
    whole = [topo_arrays(native, dev, axis, off, ref, st) for st in stations]
    tally = Tally()
    for k in range(len(stations)):
        for s in range(dev.n):
            want = scan_passes(axis, whole[k][0][s], whole[k][1][s], whole[k][2][s], np.radians(masks[k]))
            tally.whole_axis(spans(want, "grid_rise", "grid_set"), whole[k][2][s] != 0, len(axis))
    # the member is well above the mask of either station at its grid point: a set cut at g0, a rise cut at g1
    for k, g in ((2, g0), (3, g1)):
        assert whole[k][2][ROW_BAD, g] == 0 and np.radians(20.0) < whole[k][0][ROW_BAD, g, 1] < np.radians(60.0)
    worst = 0.0
    for s in range(WINDOWS):
        times = np.ascontiguousarray(axis[s:s + WINDOW])
        got, got_cnt = dev.find_passes_stations(times, off, stations, masks, reference_jd=ref, max_passes=ROOM)
        for k in range(len(stations)):
            rec, cnt = single(dev, times, off, ref, stations[k], masks[k], ROOM)
            arrays = cut(whole[k], s, s + WINDOW)
            wants, d = assert_passes(rec, cnt, times, arrays, np.radians(masks[k]))
            assert_matches(got[k], got_cnt[k], rec, cnt)
            worst = max(worst, d)
            for r in range(dev.n):
                tally.window(spans(wants[r], "grid_rise", "grid_set"), arrays[2][r] != 0, WINDOW)
    print("max |dt| against the numpy scan %.3g min" % worst)
    tally.check("passes")


def test_every_lane_eclipses(native, case, sweep):
    """find_eclipses, both kinds, on a date that puts the failing member's last good point before its failed run and its first
    after it into the umbra (test_eclipse_edge_cases' date scan, for both ends): an exit and an entry cut by the error."""
    pairs, dev, ref, off = case
    axis, g0, g1, _ = sweep
    whole = frame_arrays(native, dev, axis, off, ref, native.OUT_TEME)
    p = whole[0][ROW_BAD]
    dates = [ref + k for k in range(0, 366, 3)]
    dates = [jd for jd in dates if all(native.shadow_state(p[g], native.sun_position(jd + axis[g] / 1440.0))[0] == 2 for g in (g0, g1))]
    assert dates
    jd = dates[0]
    tab = kernel_sun(native, jd, axis)
    worst = 0.0
    for kind in (0, 1):
        tally = Tally()
        for s in range(dev.n):
            want = scan_eclipses(axis, whole[0][s], whole[1][s], whole[2][s], tab, kind)
            tally.whole_axis(spans(want, "grid_entry", "grid_exit"), whole[2][s] != 0, len(axis))
        for s in range(WINDOWS):
            times = np.ascontiguousarray(axis[s:s + WINDOW])
            rec, cnt, state = dev.find_eclipses(times, off, reference_jd=jd, kind=kind, max_eclipses=ROOM, state=True)
            arrays = cut(whole, s, s + WINDOW)
            wants, d = assert_eclipses(rec, cnt, state, times, arrays, tuple(a[s:s + WINDOW] for a in tab), kind)
            worst = max(worst, d)
            for r in range(dev.n):
                tally.window(spans(wants[r], "grid_entry", "grid_exit"), arrays[2][r] != 0, WINDOW)
        tally.check("eclipses, kind %d, Sun of JD %.1f" % (kind, jd))
    print("max |dt| against the numpy scan %.3g min" % worst)


def access_whole_axis(native, dev, off, axis, g0, g1):
    """The failing member as the target on the whole axis: (every row's scan, the grid points at which it failed, the rows in
    access to it at its last good point before the failed run, and at its first after)."""
    whole = []
    _, _, state, _, _, _ = check_against_scan(native, dev, off, axis, ROW_BAD, 0.0, None, room=ROOM, collect=whole)
    bad = state[0] == 255  # the target failed: every row fails there
    assert bad[g0 + 1:g1].all() and not bad[g0] and not bad[g1]
    # (the state matrix is the numpy scan's: check_against_scan has just held it to that)
    return whole, bad, np.flatnonzero(state[:ROW_BAD, g0] == 2), np.flatnonzero(state[:ROW_BAD, g1] == 2)


def test_every_lane_access_as_target(native, case, sweep):
    """find_access in test_decayed_member's arrangement, grazing altitude 0, the failing member as the target: the windows of
    the rows in access to it at either end of its failed run are cut there.  (The reference is check_against_scan's own
    propagation of each window: min_range_km is a grid value held to 1e-9 km, the level at which the fast step's positions
    move with the grid's segmentation.)"""
    pairs, dev, ref, off = case
    axis, g0, g1, _ = sweep
    whole, bad, before, after = access_whole_axis(native, dev, off, axis, g0, g1)
    tally = Tally()
    for s in range(ROW_BAD):
        tally.whole_axis(spans(whole[s], "grid_start", "grid_end"), bad, len(axis))
    worst = 0.0
    for s in range(WINDOWS):
        wants = []
        _, _, _, _, d, _ = check_against_scan(native, dev, off, np.ascontiguousarray(axis[s:s + WINDOW]), ROW_BAD, 0.0, None, room=ROOM,
                                              collect=wants)
        worst = max(worst, d)
        for r in range(ROW_BAD):
            tally.window(spans(wants[r], "grid_start", "grid_end"), bad[s:s + WINDOW], WINDOW)
    print("max |dt| against the numpy scan %.3g min" % worst)
    tally.check("access, the failing member as the target")


def test_every_lane_access_as_row(native, case, sweep):
    """... and as a row, in a handle that holds it and one row in access to it from either end of its failed run, each of the
    two the target in turn: its own windows are cut."""
    pairs, dev, ref, off = case
    axis, g0, g1, _ = sweep
    _, bad, before, after = access_whole_axis(native, dev, off, axis, g0, g1)
    print("rows in access to the failing member at its last good point before the run: %s, at its first after: %s" % (before, after))
    assert len(before) and len(after)
    rows = np.array([before[0], after[0], ROW_BAD], dtype=np.uint32)
    part = dev.subset(rows)
    tally = Tally()
    for tg in (0, 1):
        whole = []
        check_against_scan(native, part, off[rows], axis, tg, 0.0, None, room=ROOM, collect=whole)
        tally.whole_axis(spans(whole[2], "grid_start", "grid_end"), bad, len(axis))
    worst = 0.0
    for s in range(WINDOWS):
        for tg in (0, 1):
            wants = []
            _, _, _, _, d, _ = check_against_scan(native, part, off[rows], np.ascontiguousarray(axis[s:s + WINDOW]), tg, 0.0, None,
                                                  room=ROOM, collect=wants)
            worst = max(worst, d)
            tally.window(spans(wants[2], "grid_start", "grid_end"), bad[s:s + WINDOW], WINDOW)
    print("max |dt| against the numpy scan %.3g min" % worst)
    tally.check("access, the failing member as a row")
