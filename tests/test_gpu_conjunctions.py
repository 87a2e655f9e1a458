"""Refined close approaches on the GPU (azh_find_conjunctions_*, astroz_amd.conjunctions): the kernel against a numpy
restatement of its grid algorithm on the library's own TEME output (chunk, group, slice and window seams included), against an
independent one-second scan of the oracle propagator, the edge cases of the other finders, and the Python entry point.  The
model is restated here in numpy; the reference project has nothing to compare with."""
from datetime import datetime, timezone

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

VALUE, NULL = -20, -101
THR_SMALL, THR_LARGE, THR_ALL = 10.0, 5000.0, 40000.0  # km: the operator's screen, one with about 2,000 events (low slots), and
# one that the deep-space and geostationary slots' brackets pass too
# gates of the comparison with the one-second truth: four times the largest differences the numpy restatement shows on the
# ORACLE's own one-minute output against the oracle's one-second scan of this catalog, rounded up (see
# test_conjunctions_against_one_second_scan)
GATE_TCA_S, GATE_MISS_KM = 0.005, 0.004


@pytest.fixture(scope="module")
def synth():
    from astroz_amd import synth as s
    return s


# ---- the model in numpy ---------------------------------------------------------------------------------------------

def refine_all(d0, w0, d1, w1, dt):
    """az_ca_refine on arrays of brackets (m, 3) and interval lengths dt (m,) minutes: (sigma, miss km, speed km/s).  The
    same iteration element by element: regula falsi with the Illinois correction from the secant of the ends."""
    k = (60.0 * dt)[:, None]
    D = d1 - d0
    m0, m1 = k * w0, k * w1
    c2, c3 = 3.0 * D - 2.0 * m0 - m1, m0 + m1 - 2.0 * D

    def track(s, idx):
        s = s[:, None]
        x = d0[idx] + s * (m0[idx] + s * (c2[idx] + s * c3[idx]))
        xd = m0[idx] + s * (2.0 * c2[idx] + s * (3.0 * c3[idx]))
        return x, xd

    def f(s, idx):
        x, xd = track(s, idx)
        return (x * xd).sum(-1)
    m = len(dt)
    every = np.arange(m)
    lo, hi = np.zeros(m), np.ones(m)
    g_lo, g_hi = f(lo, every), f(hi, every)
    s = np.ones(m)
    s[~(g_lo < 0.0)] = 0.0
    act = (g_lo < 0.0) & (g_hi > 0.0)
    s[act] = 0.5
    side = np.zeros(m, dtype=np.int8)
    for _ in range(60):
        idx = np.flatnonzero(act)
        if not len(idx):
            break
        sn = (lo[idx] * g_hi[idx] - hi[idx] * g_lo[idx]) / (g_hi[idx] - g_lo[idx])
        done = np.abs(sn - s[idx]) <= 1.0e-15
        s[idx] = sn
        gs = f(sn, idx)
        stop = done | (gs == 0.0)
        act[idx[stop]] = False
        go, gsg, sg = idx[~stop], gs[~stop], sn[~stop]
        left = gsg < 0.0
        a, b = go[left], go[~left]
        lo[a], g_lo[a] = sg[left], gsg[left]
        g_hi[a] = np.where(side[a] == 1, 0.5 * g_hi[a], g_hi[a])
        side[a] = 1
        hi[b], g_hi[b] = sg[~left], gsg[~left]
        g_lo[b] = np.where(side[b] == -1, 0.5 * g_lo[b], g_lo[b])
        side[b] = -1
    x, xd = track(s, every)
    return s, np.sqrt((x * x).sum(-1)), np.sqrt((xd * xd).sum(-1)) / k[:, 0]


def scan_conjunctions(times, P, V, E, targets):
    """The definition on satellite-major TEME states P, V (n, n_times, 3) and error codes E: every bracket of every slot,
    refined.  Returns arrays (slot, sat, grid_index, tca, miss, speed) -- no threshold applied."""
    nt = len(times)
    out = [np.zeros(0, dtype=np.int64)] * 3 + [np.zeros(0)] * 3
    if nt < 2:
        return out
    parts = []
    dt_all = np.diff(times)
    for k, t in enumerate(targets):
        d, w = P - P[t], V - V[t]
        q = (d * w).sum(-1)
        ok = (E == 0) & (E[t] == 0)[None, :]
        br = ok[:, :-1] & ok[:, 1:] & (q[:, :-1] < 0.0) & (q[:, 1:] >= 0.0)
        br[t] = False
        s_idx, i_idx = np.nonzero(br)
        if not len(s_idx):
            continue
        sig, miss, speed = refine_all(d[s_idx, i_idx], w[s_idx, i_idx], d[s_idx, i_idx + 1], w[s_idx, i_idx + 1], dt_all[i_idx])
        parts.append((np.full(len(s_idx), k), s_idx, i_idx, times[i_idx] + sig * dt_all[i_idx], miss, speed))
    if not parts:
        return out
    return [np.concatenate([p[j] for p in parts]) for j in range(6)]


def as_events(scan, thr):
    """({(slot, sat, grid_index): (tca, miss, speed)} of the brackets below thr, the keys within 1e-9 km of it)."""
    slot, sat, gi, tca, miss, speed = scan
    ev, edge = {}, set()
    for j in np.flatnonzero(miss < thr + 1e-9):
        key = (int(slot[j]), int(sat[j]), int(gi[j]))
        if abs(miss[j] - thr) <= 1e-9:
            edge.add(key)
        elif miss[j] < thr:
            ev[key] = (tca[j], miss[j], speed[j])
    return ev, edge


def keyed(rec):
    out = {(int(r["target"]), int(r["sat"]), int(r["grid_index"])): (float(r["t_tca_min"]), float(r["miss_km"]), float(r["rel_speed_km_s"]))
           for r in rec}
    assert len(out) == len(rec)  # no event twice
    return out


def check_against_scan(rec, n_ev, scan, thr, what=""):
    """The device's records against the restatement: equal key sets (events within 1e-9 km of the threshold left out and
    counted, at most 1 %), tca within 1e-9 min, miss and speed within 1e-9 km and km/s, reserved == 0."""
    assert n_ev == len(rec), (what, n_ev, len(rec))
    assert not rec["reserved"].any()
    want, edge = as_events(scan, thr)
    got = keyed(rec)
    for key in edge:
        got.pop(key, None)
    assert len(edge) <= 0.01 * max(len(want), 1) or not want, (what, len(edge), len(want))
    assert set(got) == set(want), (what, sorted(set(got) - set(want))[:5], sorted(set(want) - set(got))[:5])
    worst = [0.0, 0.0, 0.0]
    for key, w in want.items():
        g = got[key]
        err = [abs(g[j] - w[j]) for j in range(3)]
        worst = [max(a, b) for a, b in zip(worst, err)]
        assert max(err) <= 1e-9, (what, key, g, w)
    return len(want), len(edge), worst


# ---- the catalog of the grid and oracle checks -------------------------------------------------------------------------

LOW = dict(incl=53.0, raan=120.0, ecc=0.001, argp=30.0, ma=40.0, mm=15.05, bstar=1e-5)


def conjunction_pairs(synth):
    """About 200 synthetic near-earth rows, the three reference deep-space members, one eccentric member and one
    geostationary member (test_gpu_eclipse's catalog), and behind them an engineered low target (row 202) with its partners:
    the same elements with the node moved by 0.05 degrees (203: side by side, closest twice a revolution at the highest
    latitudes) or the inclination by 0.2 degrees (204: crossing at the nodes, slowly), the mirrored inclination (205: meeting
    head-on at both nodes at 9 km/s), and an exact duplicate (206)."""
    pairs = synth.synth_catalog(n_near=197, n_deep=3, seed=41)
    pairs.append(synth.format_tle(99001, synth.START_JD, 63.4, 40.0, 0.25, 270.0, 10.0, 9.0, 1e-5))
    pairs.append(synth.format_tle(99002, synth.START_JD, 0.05, 0.0, 0.0002, 0.0, 0.0, 1.00273791, 0.0))

    def low(num, **kw):
        e = dict(LOW, **kw)
        return synth.format_tle(num, synth.START_JD, e["incl"], e["raan"], e["ecc"], e["argp"], e["ma"], e["mm"], e["bstar"])
    pairs += [low(99010), low(99011, raan=120.05), low(99012, incl=53.2), low(99013, incl=127.0), low(99010)]
    return pairs


ROW_ECC, ROW_GEO, ROW_LOW, ROW_DUP = 200, 201, 202, 206


def mean_motions(pairs):
    return np.array([float(l2[52:63]) for _, l2 in pairs])


def target_slots(pairs):
    """A low row, the eccentric one, a deep-space one, the geostationary one, a row given twice, a low row of the synthetic mix."""
    mm = mean_motions(pairs[:200])
    deep, near = int(np.flatnonzero(mm < 6.0)[0]), int(np.flatnonzero(mm > 14.0)[0])
    return [ROW_LOW, ROW_ECC, deep, ROW_GEO, ROW_LOW, near]


@pytest.fixture(scope="module")
def case(native, synth):
    """The catalog on the device, six hours of one-minute steps, the library's own TEME states and the restated scan."""
    pairs = conjunction_pairs(synth)
    dev = native.DeviceConstellation.from_tle_lines(pairs, 0, 0)
    ref = synth.START_JD
    off = (ref - dev.epochs) * 1440.0
    times = np.arange(0.0, 360.0)
    targets = target_slots(pairs)
    P, V, E = host_states(native, dev, times, off)
    scan = scan_conjunctions(times, P, V, E, targets)
    return pairs, dev, off, times, targets, scan


def host_states(native, dev, times, off):
    n, nt = dev.n, len(times)
    P, V = np.empty((n, nt, 3)), np.empty((n, nt, 3))
    E = np.zeros((n, nt), dtype=np.uint8)
    if nt:
        dev.propagate_host(times, off, pos=P, vel=V, mode=native.OUT_TEME, layout=native.SAT_MAJOR, err=E)
    return P, V, E


def test_conjunctions_match_grid_algorithm(native, case):
    pairs, dev, off, times, targets, scan = case
    assert dev.n == 207 and len(targets) == 6
    for thr, floor in ((THR_SMALL, 20), (THR_LARGE, 1200), (THR_ALL, 5000)):
        rec, n_ev = dev.find_conjunctions(times, targets, thr, off, max_events=20000)
        n, n_edge, worst = check_against_scan(rec, n_ev, scan, thr)
        print("threshold %g km: %d events (%d within 1e-9 km of it), max |d tca| %.3g min, |d miss| %.3g km, |d speed| %.3g km/s"
              % (thr, n, n_edge, *worst))
        assert n > floor
        got = keyed(rec)
        # the slot given twice reports what its twin does; a slot's own row and its exact duplicate report nothing
        twin = {k[1:]: v for k, v in got.items() if k[0] == 0}
        assert twin and twin == {k[1:]: v for k, v in got.items() if k[0] == 4}
        for (slot, sat, _i) in got:
            assert sat != targets[slot] and not (targets[slot] == ROW_LOW and sat == ROW_DUP)
        assert {k[1] for k in got if k[0] == 0} >= ({203, 204, 205} if thr == THR_SMALL else set())
        # the host list is sorted by (target, sat, tca)
        order = np.lexsort((rec["t_tca_min"], rec["sat"], rec["target"]))
        assert np.array_equal(order, np.arange(len(rec)))


@pytest.mark.parametrize("n_times", [2, 63, 64, 65, 127, 190])
def test_chunk_group_and_slice_edges(native, case, n_times):
    """Chunks advance by 63 points: with these grids a bracket falls on every chunk seam; 1 / 16 / 17 / 33 slots for the seam
    between target groups; the 207 rows are sliced eight at a time."""
    pairs, dev, off, _t, _targets, _scan = case
    rng = np.random.default_rng(n_times)
    for axis in ("regular", "jitter"):
        times = np.arange(0.0, float(n_times))
        if axis == "jitter":
            times = times + rng.uniform(-1.0 / 3, 1.0 / 3, n_times)  # one-minute steps with +-20 s
            assert (np.diff(times) > 0).all()
        P, V, E = host_states(native, dev, times, off)
        for K in (1, 16, 17, 33):
            targets = [ROW_LOW] + [int(x) for x in rng.choice(dev.n, K - 1)]
            scan = scan_conjunctions(times, P, V, E, targets)
            rec, n_ev = dev.find_conjunctions(times, targets, THR_LARGE, off, max_events=60000)
            n, n_edge, worst = check_against_scan(rec, n_ev, scan, THR_LARGE, (n_times, axis, K))
            seams = sorted({k[2] for k in keyed(rec) if k[2] % 63 in (62, 0)})
            print("%d times, %s, %d slots: %d events, seam intervals %s" % (n_times, axis, K, n, seams[:6]))
            if n_times > 64 and K >= 16:
                assert {62, 63} <= set(seams)


def test_no_grid_interval(native, case):
    pairs, dev, off, times, targets, scan = case
    for n_times in (0, 1):
        rec, n_ev = dev.find_conjunctions(times[:n_times], targets, THR_LARGE, off, max_events=8)
        assert n_ev == 0 and len(rec) == 0


# ---- against the truth -----------------------------------------------------------------------------------------------

def truth_minima(fine, p_t, v_t, p_s, v_s):
    """Local minima of |d| on the one-second axis `fine` (minutes), each refined by the parabola through the three samples
    of |d|^2 around it (exact for straight relative motion, where a parabola through samples of |d| itself would miss the tip
    of the V): (t_min minutes, miss km, index of the sample)."""
    d = p_s - p_t
    d2 = (d * d).sum(-1)
    j = np.flatnonzero((d2[1:-1] <= d2[:-2]) & (d2[1:-1] < d2[2:])) + 1
    a, b, c = d2[j - 1], d2[j], d2[j + 1]
    den = a - 2.0 * b + c
    x = np.where(den > 0, 0.5 * (a - c) / np.where(den > 0, den, 1.0), 0.0)  # in samples, |x| <= 1/2
    m2 = b - 0.125 * (a - c) ** 2 / np.where(den > 0, den, 1.0)
    return fine[j] + x / 60.0, np.sqrt(np.maximum(m2, 0.0)), j


def one_second_truth(orc, pairs, off, times, targets, thr):
    """{slot: [(t_min, miss, regular bracket?, sat)]} of every truth minimum below thr + 1 km, from the oracle at one second,
    in blocks of 25 rows."""
    fine = np.arange(0.0, times[-1] * 60.0 + 0.5) / 60.0
    uniq = sorted(set(targets))
    tcat = orc.Catalog.from_pairs([pairs[t] for t in uniq], 0)
    et, pt, vt = tcat.propagate(fine, off[uniq], mode=orc.TEME, threads=16)
    out = {k: [] for k in range(len(targets))}
    n = len(pairs)
    for lo in range(0, n, 25):
        hi = min(n, lo + 25)
        sub = orc.Catalog.from_pairs(pairs[lo:hi], 0)
        e0, p0, v0 = sub.propagate(fine, off[lo:hi], mode=orc.TEME, threads=16)
        for k, t in enumerate(targets):
            u = uniq.index(t)
            for s in range(lo, hi):
                if s == t:
                    continue
                tm, miss, j = truth_minima(fine, pt[u], vt[u], p0[s - lo], v0[s - lo])
                for a in np.flatnonzero(miss < thr + 1.0):
                    i = min(int(np.floor(tm[a])), len(times) - 2)  # the grid interval [i, i + 1] that holds it
                    g0, g1 = 60 * i, 60 * (i + 1)
                    q0 = np.dot(p0[s - lo, g0] - pt[u, g0], v0[s - lo, g0] - vt[u, g0])
                    q1 = np.dot(p0[s - lo, g1] - pt[u, g1], v0[s - lo, g1] - vt[u, g1])
                    ok = not (e0[s - lo, g0] or e0[s - lo, g1] or et[u, g0] or et[u, g1])
                    inside = bool(ok and tm[a] > times[0] and tm[a] < times[-1])
                    out[k].append((float(tm[a]), float(miss[a]), bool(inside and q0 < 0.0 and q1 >= 0.0), s))
    return out


def test_conjunctions_against_one_second_scan(native, orc, case):
    """Every reported event is one true minimum of the oracle's one-second scan and no true minimum is matched twice; tca within
    GATE_TCA_S and miss within GATE_MISS_KM of it.  Every true minimum further below the threshold than the miss gate that
    has a regular bracket (both grid neighbours propagated, d.w changing sign across the interval) is reported.

    The gates, measured with the oracle alone (the numpy restatement on the oracle's one-minute output against the oracle's
    one-second minima, this catalog, START_JD, 10 km, 44 events): largest |d tca| 0.00111 s (the side-by-side partner, whose
    distance has a flat minimum), largest |d miss| 0.00086 km (the head-on partner at 9.1 km/s); four times those, rounded up:
    0.005 s and 0.004 km.  True minima below the threshold without a regular bracket (out of a grid scan's reach): counted,
    cap 2 %; 0 of 44 in the same measurement."""
    pairs, dev, off, times, targets, scan = case
    thr = THR_SMALL
    rec, n_ev = dev.find_conjunctions(times, targets, thr, off, max_events=4096)
    assert n_ev == len(rec) > 20
    truth = one_second_truth(orc, pairs, off, times, targets, thr)
    used = set()
    worst = [0.0, 0.0]
    for r in rec:
        k, s, i = int(r["target"]), int(r["sat"]), int(r["grid_index"])
        cand = [(q, t) for q, t in enumerate(truth[k]) if t[3] == s and times[i] - GATE_TCA_S / 60 <= t[0] <= times[i + 1] + GATE_TCA_S / 60]
        assert len(cand) == 1 and (k, cand[0][0]) not in used, (r, cand)
        used.add((k, cand[0][0]))
        t = cand[0][1]
        dt_s, dm = abs(float(r["t_tca_min"]) - t[0]) * 60.0, abs(float(r["miss_km"]) - t[1])
        worst = [max(worst[0], dt_s), max(worst[1], dm)]
        assert dt_s <= GATE_TCA_S and dm <= GATE_MISS_KM, (r, t)
    n_true = n_unseen = 0
    for k in truth:
        for q, t in enumerate(truth[k]):
            if t[1] < thr:
                n_true += 1
                n_unseen += 0 if t[2] else 1
            if t[1] < thr - GATE_MISS_KM and t[2]:
                assert (k, q) in used, (k, t)
    print("%d events, %d true minima below %g km, %d without a regular bracket; max |d tca| %.4f s, |d miss| %.5f km"
          % (len(rec), n_true, thr, n_unseen, *worst))
    assert n_unseen <= 0.02 * n_true


# ---- edge cases ------------------------------------------------------------------------------------------------------

def test_conjunction_edge_cases(native, synth, case):
    import torch
    pairs, dev, off, times, targets, scan = case
    full, n_full = dev.find_conjunctions(times, targets, THR_LARGE, off, max_events=20000)
    all_keys = set(keyed(full))
    # room for fewer records than there are events: the true count, and stored records out of the full set
    few, n_few = dev.find_conjunctions(times, targets, THR_LARGE, off, max_events=100)
    assert n_few == n_full and len(few) == 100 and set(keyed(few)) <= all_keys
    none, n_none = dev.find_conjunctions(times, targets, THR_LARGE, off, max_events=0)
    assert n_none == n_full and len(none) == 0
    # _device on torch buffers and a foreign stream: the same set
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d_out = torch.zeros(20000 * 40, dtype=torch.uint8, device="cuda")
        d_n = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    stream.synchronize()
    dev.find_conjunctions_device(times, targets, THR_LARGE, off, d_out.data_ptr(), 20000, d_n.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    assert int(d_n.cpu()[0]) == n_full
    got = d_out.cpu().numpy().view(native.CONJUNCTION_DTYPE)[:n_full]
    assert keyed(got) == keyed(full)
    # the argument codes
    L = native.lib()
    t = np.ascontiguousarray(times[:8])
    tg = np.array(targets, dtype=np.uintp)
    cnt = np.full(1, 9, dtype=np.uint32)

    def call(tt=t, thr=10.0, tgs=tg, n_tg=None, room=0, out=None, cnt_p=cnt.ctypes.data, tg_p=True):
        return L.azh_find_conjunctions_host(dev._h, tt.ctypes.data, len(tt), off.ctypes.data, tgs.ctypes.data if tg_p else None,
                                            len(tgs) if n_tg is None else n_tg, thr, out, room, cnt_p)
    assert call() == 0
    for bad_t in (np.array([0.0, 1.0, 1.0]), np.array([2.0, 1.0]), np.array([0.0, np.nan, 2.0])):
        assert call(tt=bad_t) == VALUE
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert call(thr=bad) == VALUE
    assert call(tgs=np.array([0, dev.n], dtype=np.uintp)) == VALUE and call(tgs=np.array([dev.n - 1], dtype=np.uintp)) == 0
    assert call(n_tg=0) == VALUE and call(room=1 << 32) == VALUE
    assert call(room=4) == NULL and call(cnt_p=None) == NULL and call(tg_p=False) == NULL
    cnt[:] = 7
    assert call(tt=t[:1]) == 0 and cnt[0] == 0  # no grid interval: a zero count
    one = np.zeros(1, dtype=np.uint32)
    assert L.azh_find_conjunctions_device(dev._h, t.ctypes.data, len(t), off.ctypes.data, tg.ctypes.data, len(tg), 10.0, None, 0, None,
                                          None) == NULL
    assert L.azh_find_conjunctions_device(dev._h, t.ctypes.data, len(t), off.ctypes.data, tg.ctypes.data, len(tg), -1.0, None, 0,
                                          one.ctypes.data, None) == VALUE


def test_member_that_fails_mid_grid(native, synth, case):
    """A member whose propagation fails mid-grid (test_gpu_eclipse's 99100), as a row and as a target: no event on a bracket
    touching a failed point, and the events of every other pair unchanged."""
    pairs, _dev, off, _times, targets, _scan = case
    dev = native.DeviceConstellation.from_tle_lines(pairs, 0, 0)
    dev.set_time_tile(256, 256)  # (both handles cut the day into the same time segments: test_gpu_access's reason)
    times = np.arange(0.0, 1440.0)
    bad = synth.format_tle(99100, synth.START_JD, 63.4, 10.0, 0.49, 270.0, 0.0, 6.1, 0.01)
    both = native.DeviceConstellation.from_tle_lines(pairs + [bad], 0, 0)
    both.set_time_tile(256, 256)
    off2 = (synth.START_JD - both.epochs) * 1440.0
    P, V, E = host_states(native, both, times, off2)
    row = both.n - 1
    fail = int(np.flatnonzero(E[row])[0])
    assert 10 < fail < len(times) - 10 and not E[row, :fail].any() and not E[:row].any()
    tg = [ROW_LOW, row, ROW_ECC]
    thr = 20000.0  # (the failing member is high and eccentric: few rows come within THR_LARGE of it)
    rec, n_ev = both.find_conjunctions(times, tg, thr, off2, max_events=60000)
    n, n_edge, _ = check_against_scan(rec, n_ev, scan_conjunctions(times, P, V, E, tg), thr)
    got = keyed(rec)
    with_bad = [k for k in got if k[0] == 1 or k[1] == row]
    assert len(with_bad) > 50
    for k in with_bad:
        assert not E[row, k[2]] and not E[row, k[2] + 1]
    base, n_base = dev.find_conjunctions(times, [ROW_LOW, ROW_LOW, ROW_ECC], thr, off, max_events=60000)
    rest = {k: v for k, v in got.items() if k[0] != 1 and k[1] != row}
    want = {k: v for k, v in keyed(base).items() if k[0] != 1}
    assert set(rest) == set(want) and n_base == len(base)
    assert max(abs(rest[k][j] - want[k][j]) for k in want for j in range(3)) <= 1e-9


def test_several_row_windows(native, synth):
    """13,478 x 1,440: the scratch takes two row windows (7,608 rows each), so the targets' tracks come from row-window launches
    of their own (one per run of consecutive rows) instead of the scratch: a run of two targets in the first window, one target
    in the second.  The events of the second window's rows against a handle that holds only them and the first window's
    targets (one window: tracks out of the scratch)."""
    pairs = synth.synth_catalog(13478, 0)
    dev = native.DeviceConstellation.from_tle_lines(pairs, native.WGS72, 0)
    dev.set_time_tile(256, 256)  # (both handles cut the day into the same time segments: test_gpu_access's reason)
    times = np.arange(1440.0)
    off = (synth.START_JD - dev.epochs) * 1440.0
    tg = [100, 10000, 101]
    rec, n_ev = dev.find_conjunctions(times, tg, 50.0, off, max_events=200000)
    assert n_ev == len(rec)
    rows = np.concatenate([[100, 101], np.arange(7000, 13478)]).astype(np.uint32)
    part = dev.subset(rows)
    part.set_time_tile(256, 256)
    r2, n2 = part.find_conjunctions(times, [0, 3002, 1], 50.0, off[rows], max_events=200000)
    assert n2 == len(r2)
    a = {k: v for k, v in keyed(rec).items() if k[1] >= 7000}
    b = {(k[0], int(rows[k[1]]), k[2]): v for k, v in keyed(r2).items() if k[1] >= 2}
    print("%d events in all, %d in rows 7000 and up (slots: %s)" % (n_ev, len(a), sorted({k[0] for k in a})))
    assert len(a) > 20 and {k[0] for k in a} == {0, 1, 2} and any(k[1] >= 7608 for k in a)
    assert set(a) == set(b)
    assert max(abs(a[k][j] - b[k][j]) for k in a for j in range(3)) <= 1e-9


def test_python_end_to_end(native, synth):
    import astroz_amd
    pairs = synth.synth_catalog(n_near=40, seed=77)
    e = dict(LOW)
    pairs.append(synth.format_tle(99010, synth.START_JD, e["incl"], e["raan"], e["ecc"], e["argp"], e["ma"], e["mm"], e["bstar"]))
    pairs.append(synth.format_tle(99012, synth.START_JD, e["incl"] + 0.2, e["raan"], e["ecc"], e["argp"], e["ma"], e["mm"], e["bstar"]))
    pairs.append(synth.format_tle(99013, synth.START_JD, 127.0, e["raan"], e["ecc"], e["argp"], e["ma"], e["mm"], e["bstar"]))
    text = synth.pairs_to_text(pairs)
    const = astroz_amd.Constellation(text)
    when = datetime.fromtimestamp((synth.START_JD - 2440587.5) * 86400.0, tz=timezone.utc)
    start = astroz_amd._jd_of(when)
    off = (start - const._dev.epochs) * 1440.0
    times = np.arange(0.0, 720.0)
    ev = astroz_amd.conjunctions(text, times, [40, 3], 10.0, start_time=when)
    assert ev.dtype == astroz_amd.CONJUNCTION_DTYPE and ev.dtype.names == ("target", "sat", "tca", "miss", "rel_speed", "grid_index")
    assert len(ev) > 10 and set(ev["target"]) <= {40, 3} and 40 in ev["target"]  # the row, not the slot
    assert {41, 42} <= set(ev["sat"][ev["target"] == 40])
    assert np.array_equal(np.lexsort((ev["tca"], ev["sat"], ev["target"])), np.arange(len(ev)))
    assert (ev["miss"] < 10.0).all() and (ev["tca"] >= times[ev["grid_index"]]).all() and (ev["tca"] <= times[ev["grid_index"] + 1]).all()
    # the same rows from the native call (slots 0, 1 = rows 40, 3)
    rec, n_ev = const._dev.find_conjunctions(times, [40, 3], 10.0, off, max_events=1000)
    assert n_ev == len(ev) == len(rec)
    rec = rec[np.lexsort((rec["t_tca_min"], rec["sat"], np.array([40, 3])[rec["target"]]))]
    assert np.array_equal(ev["tca"], rec["t_tca_min"]) and np.array_equal(ev["miss"], rec["miss_km"])
    assert np.array_equal(ev["rel_speed"], rec["rel_speed_km_s"]) and np.array_equal(ev["sat"], rec["sat"])
    assert np.array_equal(ev["grid_index"], rec["grid_index"])
    one = astroz_amd.conjunctions(const, times, 40, start_time=when)  # an int, the default threshold
    assert np.array_equal(one, ev[ev["target"] == 40])
    # more events than the wrapper's first room: every row a target, a threshold no pair escapes
    every = astroz_amd.conjunctions(const, times, np.arange(const.num_satellites), 1.0e5, start_time=when)
    rec, n_ev = const._dev.find_conjunctions(times, np.arange(const.num_satellites), 1.0e5, off, max_events=0)
    assert len(every) == n_ev > astroz_amd._CONJUNCTION_ROOM
    assert np.array_equal(np.lexsort((every["tca"], every["sat"], every["target"])), np.arange(len(every)))
    for bad in ([43], [0, 43], 43):
        with pytest.raises(ValueError):
            astroz_amd.conjunctions(const, times, bad, start_time=when)
    with pytest.raises(ValueError):
        astroz_amd.conjunctions(const, times[::-1], 0, start_time=when)
    with pytest.raises(ValueError):
        astroz_amd.conjunctions(const, times, 0, -5.0, start_time=when)
