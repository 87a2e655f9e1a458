"""CPU tier of the conjunction finder: the host twin of the closest-approach model (a pure host export) against the analytic
answer on straight relative tracks and against an extended-precision restatement of the same Hermite on two-body pairs, the ABI
of azh_conjunction, and the argument checks that need no device."""
import ctypes as C
import re

import numpy as np
import pytest

VALUE, NULL = -20, -101
MU = 398600.8


def _twin(L, d0, w0, d1, w1, dt):
    a, b, c, d = (np.ascontiguousarray(x, dtype=np.float64) for x in (d0, w0, d1, w1))
    s, m, v = C.c_double(-7.0), C.c_double(-7.0), C.c_double(-7.0)
    rc = L.azh_closest_approach(a.ctypes.data, b.ctypes.data, c.ctypes.data, d.ctypes.data, float(dt), C.addressof(s), C.addressof(m),
                                C.addressof(v))
    return rc, s.value, m.value, v.value


def longdouble_approach(d0, w0, d1, w1, dt):
    """(sigma, miss, speed) of the model in extended precision: the cubic Hermite of d with end slopes 60 dt w, and the root
    of d.d' in [0, 1] by bisection down to the last bit."""
    ld = np.longdouble
    d0, w0, d1, w1 = (np.asarray(x, dtype=ld) for x in (d0, w0, d1, w1))
    k = ld(60) * ld(dt)
    m0, m1, D = k * w0, k * w1, d1 - d0
    c2, c3 = 3 * D - 2 * m0 - m1, m0 + m1 - 2 * D

    def track(s):
        return d0 + s * (m0 + s * (c2 + s * c3)), m0 + s * (2 * c2 + s * 3 * c3)

    def f(s):
        x, xd = track(s)
        return (x * xd).sum()
    lo, hi = ld(0), ld(1)
    assert f(lo) < 0 <= f(hi)
    for _ in range(80):
        mid = (lo + hi) / 2
        if f(mid) < 0:
            lo = mid
        else:
            hi = mid
    x, xd = track(hi)
    return hi, np.sqrt((x * x).sum()), np.sqrt((xd * xd).sum()) / k


def test_symbols_and_abi(native):
    L = native.lib()
    for name in ("azh_closest_approach", "azh_find_conjunctions_host", "azh_find_conjunctions_device"):
        assert hasattr(L, name) and name in native.EXPORTS
    hdr = open(native.os.path.join(native._HERE, "..", "include", "astroz_hip.h")).read()
    m = re.search(r"typedef struct azh_conjunction \{(.*?)\} azh_conjunction;", hdr, flags=re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [f.strip() for decl in body.split(";") if decl.strip() for f in decl.split(None, 1)[1].split(",")]
    assert fields == list(native.CONJUNCTION_DTYPE.names)

    class Conjunction(C.Structure):  # the header's declaration, laid out by the C rules
        _fields_ = [("t_tca_min", C.c_double), ("miss_km", C.c_double), ("rel_speed_km_s", C.c_double), ("target", C.c_uint32),
                    ("sat", C.c_uint32), ("grid_index", C.c_uint32), ("reserved", C.c_uint32)]
    assert C.sizeof(Conjunction) == 40 and native.CONJUNCTION_DTYPE.itemsize == 40
    want = {"t_tca_min": 0, "miss_km": 8, "rel_speed_km_s": 16, "target": 24, "sat": 28, "grid_index": 32, "reserved": 36}
    for name, off in want.items():
        assert getattr(Conjunction, name).offset == off and native.CONJUNCTION_DTYPE.fields[name][1] == off, name


def test_straight_line_is_exact(native):
    """Uniform relative motion d(t) = p + u (t - t_c): the Hermite IS the track, so sigma, miss and speed are the analytic
    ones: 1e-12 in sigma, 1e-9 km, and the speed to 1e-12 relative."""
    L = native.lib()
    rng = np.random.default_rng(3)
    worst = [0.0, 0.0, 0.0]
    n = 0
    for _ in range(3000):
        dt = rng.uniform(0.5, 2.0)
        k = 60.0 * dt
        u = rng.normal(size=3)
        u *= rng.uniform(0.05, 15.0) / np.linalg.norm(u)  # km/s (sigma is conditioned like eps |p| / (k |u|) <= 1e-13)
        p = np.cross(u, rng.normal(size=3))
        p *= 10.0 ** rng.uniform(-3, 3) / np.linalg.norm(p)  # the miss vector, perpendicular to u
        sig = rng.uniform(0.0, 1.0)
        d0, d1 = p - u * (sig * k), p + u * ((1.0 - sig) * k)
        if not (np.dot(d0, u) < 0 <= np.dot(d1, u)):
            continue
        # the analytic answer for the inputs as rounded
        s_true = -np.dot(d0, u) / (np.dot(u, u) * k)
        miss_true = np.linalg.norm(np.cross(d0, u)) / np.linalg.norm(u)
        rc, s, miss, v = _twin(L, d0, u, d1, u, dt)
        assert rc == 1
        n += 1
        worst = [max(worst[0], abs(s - s_true)), max(worst[1], abs(miss - miss_true)), max(worst[2], abs(v / np.linalg.norm(u) - 1))]
        assert abs(s - s_true) <= 1e-12 and abs(miss - miss_true) <= 1e-9 and abs(v / np.linalg.norm(u) - 1) <= 1e-12, (d0, u, dt)
        assert native.closest_approach(d0, u, d1, u, dt) == (s, miss, v)
    print("%d straight tracks: max |d sigma| %.3g, |d miss| %.3g km, relative |d speed| %.3g" % (n, *worst))
    assert n > 2500


def test_head_on_and_no_bracket(native):
    L = native.lib()
    # head-on: through the origin at sigma = 0.25
    u = np.array([3.0, -4.0, 12.0])  # 13 km/s
    d0, d1 = -u * 15.0, u * 45.0
    rc, s, miss, v = _twin(L, d0, u, d1, u, 1.0)
    assert rc == 1 and abs(s - 0.25) <= 1e-12 and miss <= 1e-9 and abs(v - 13.0) <= 1e-11
    # the minimum exactly at the right end (q1 == 0) is a bracket; exactly at the left end (q0 == 0) is not
    p = np.array([0.0, 5.0, 0.0])
    ux = np.array([2.0, 0.0, 0.0])
    rc, s, miss, v = _twin(L, p - ux * 60.0, ux, p, ux, 1.0)
    assert rc == 1 and s == 1.0 and miss == 5.0 and v == 2.0
    for d0, w0, d1, w1 in ((p, ux, p + ux * 60.0, ux),                      # q0 == 0
                           (p + ux * 60.0, ux, p + ux * 120.0, ux),          # receding: q0 > 0
                           (p - ux * 120.0, ux, p - ux * 60.0, ux),          # closing at both ends: q1 < 0
                           (np.zeros(3), np.zeros(3), np.zeros(3), np.zeros(3)),  # the same object twice: q == 0
                           (p - ux, ux, p * np.nan, ux)):                    # not a number: no bracket
        rc, s, miss, v = _twin(L, d0, w0, d1, w1, 1.0)
        assert rc == 0 and (s, miss, v) == (-7.0, -7.0, -7.0)  # outputs untouched
        assert native.closest_approach(d0, w0, d1, w1, 1.0) is None
    a = np.ones(3)
    for args in ((None, a, a, a), (a, None, a, a), (a, a, None, a), (a, a, a, None)):
        ptr = [None if x is None else x.ctypes.data for x in args]
        assert L.azh_closest_approach(*ptr, 1.0, None, None, None) == -1
    for dt in (0.0, -1.0, float("nan"), float("inf")):
        assert L.azh_closest_approach(a.ctypes.data, a.ctypes.data, a.ctypes.data, a.ctypes.data, dt, None, None, None) == -1
        with pytest.raises(ValueError):
            native.closest_approach(a, a, a, a, dt)
    # the output pointers are optional
    assert L.azh_closest_approach((p - ux * 60.0).ctypes.data, ux.ctypes.data, p.ctypes.data, ux.ctypes.data, 1.0, None, None, None) == 1


def _circular(a, inc, node, u):
    """State on a circular two-body orbit of radius a: inclination, node and argument of latitude in radians."""
    n = np.sqrt(MU / a ** 3)
    cu, su, ci, si, cn, sn = np.cos(u), np.sin(u), np.cos(inc), np.sin(inc), np.cos(node), np.sin(node)
    r = a * np.array([cn * cu - sn * su * ci, sn * cu + cn * su * ci, su * si])
    v = a * n * np.array([-cn * su - sn * cu * ci, -sn * su + cn * cu * ci, cu * si])
    return r, v, n


def test_two_body_pairs_match_extended_precision(native):
    """Pairs of circular orbits sampled a grid step apart: the twin against the longdouble restatement of the same Hermite,
    1e-9 km in the miss (and 1e-9 in sigma, 1e-9 km/s in the speed)."""
    L = native.lib()
    rng = np.random.default_rng(8)
    n_br, worst = 0, [0.0, 0.0, 0.0]
    for _ in range(400):
        a1, a2 = rng.uniform(6700.0, 8000.0), rng.uniform(6700.0, 8000.0)
        if rng.uniform() < 0.3:
            a2 = a1 + rng.uniform(-5.0, 5.0)  # near misses at the crossings of the two planes
        i1, i2 = rng.uniform(0.0, np.pi, 2)
        o1, o2 = rng.uniform(0.0, 2 * np.pi, 2)
        u1, u2 = rng.uniform(0.0, 2 * np.pi, 2)
        dt = rng.uniform(0.3, 1.5)
        prev = None
        for step in range(80):
            t = step * dt * 60.0
            ra, va, _ = _circular(a1, i1, o1, u1 + np.sqrt(MU / a1 ** 3) * t)
            rb, vb, _ = _circular(a2, i2, o2, u2 + np.sqrt(MU / a2 ** 3) * t)
            cur = (ra - rb, va - vb)
            if prev is not None:
                q0, q1 = np.dot(*prev), np.dot(*cur)
                rc, s, miss, v = _twin(L, prev[0], prev[1], cur[0], cur[1], dt)
                assert rc == (1 if (q0 < 0 <= q1) else 0)
                if rc:
                    ws, wm, wv = longdouble_approach(prev[0], prev[1], cur[0], cur[1], dt)
                    err = (abs(s - float(ws)), abs(miss - float(wm)), abs(v - float(wv)))
                    worst = [max(a, b) for a, b in zip(worst, err)]
                    assert err[0] <= 1e-9 and err[1] <= 1e-9 and err[2] <= 1e-9, (a1, a2, step, err)
                    n_br += 1
            prev = cur
    print("%d brackets: max |d sigma| %.3g, |d miss| %.3g km, |d speed| %.3g km/s" % (n_br, *worst))
    assert n_br > 300


def test_null_pointers_and_value_errors(native):
    """The paths that return before a handle or a device is touched."""
    L = native.lib()
    cnt = np.zeros(1, dtype=np.uint32)
    t = np.arange(4.0)
    tg = np.zeros(2, dtype=np.uintp)

    def host(times=t, thr=10.0, n_tg=2, room=0, tg_p=tg.ctypes.data, cnt_p=cnt.ctypes.data):
        return L.azh_find_conjunctions_host(None, times.ctypes.data, len(times), None, tg_p, n_tg, thr, None, room, cnt_p)

    def device(times=t, thr=10.0, n_tg=2, room=0, tg_p=tg.ctypes.data, cnt_p=cnt.ctypes.data):
        return L.azh_find_conjunctions_device(None, times.ctypes.data, len(times), None, tg_p, n_tg, thr, None, room, cnt_p, None)
    for call in (host, device):
        assert call() == NULL  # no handle
        for bad_t in (np.array([0.0, 1.0, 1.0]), np.array([2.0, 1.0]), np.array([0.0, np.nan, 2.0])):
            assert call(times=bad_t) == VALUE
        for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
            assert call(thr=bad) == VALUE
        assert call(n_tg=0) == VALUE
        assert call(room=1 << 32) == VALUE and call(room=0xffffffff) == NULL
        assert call(n_tg=1 << 62) == VALUE  # sizes that overflow


def test_python_argument_checks(native, monkeypatch):
    import astroz_amd
    assert {"conjunctions", "CONJUNCTION_DTYPE"} <= set(astroz_amd.__all__)
    assert astroz_amd.CONJUNCTION_DTYPE.names == ("target", "sat", "tca", "miss", "rel_speed", "grid_index")

    def no_handle(*a, **k):
        raise AssertionError("argument errors must be raised before a constellation is built")
    monkeypatch.setattr(astroz_amd, "Constellation", no_handle)
    good = [0.0, 1.0]
    for times in ([0.0, 1.0, 1.0], [2.0, 1.0], [0.0, np.nan, 2.0], [[0.0, 1.0], [2.0, 3.0]]):
        with pytest.raises(ValueError):
            astroz_amd.conjunctions("x", times, 0)
    for thr in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            astroz_amd.conjunctions("x", good, 0, thr)
    for targets in ([], None, -1, [0, -1], 1.5, [0, 1.5], "first", [[0, 1]], True):
        with pytest.raises(ValueError):
            astroz_amd.conjunctions("x", good, targets)
