"""CPU tier of the access finder: the host twin of the line-of-sight geometry (a pure host export) against an extended-precision
restatement, the ABI of azh_access, and the argument checks that need no device."""
import ctypes as C
import re

import numpy as np
import pytest

R_EARTH = 6378.137
VALUE, NULL = -20, -101


def longdouble_los(r1, r2):
    """(clearance, range, tau) of the segment r1-r2 by the formulas of the model, in extended precision."""
    r1, r2 = np.asarray(r1, dtype=np.longdouble), np.asarray(r2, dtype=np.longdouble)
    d = r2 - r1
    d2 = (d * d).sum()
    rng = np.sqrt(d2)
    if d2 == 0:
        return np.sqrt((r1 * r1).sum()), rng, np.longdouble(0)
    tau = -(r1 * d).sum() / d2
    if tau <= 0:
        return np.sqrt((r1 * r1).sum()), rng, tau
    if tau >= 1:
        return np.sqrt((r2 * r2).sum()), rng, tau
    c = np.cross(r1, r2)
    return np.sqrt((c * c).sum()) / rng, rng, tau


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def test_symbols_and_abi(native):
    L = native.lib()
    for name in ("azh_line_of_sight", "azh_find_access_host", "azh_find_access_device", "azh_find_access_track_device"):
        assert hasattr(L, name) and name in native.EXPORTS
    hdr = open(native.os.path.join(native._HERE, "..", "include", "astroz_hip.h")).read()
    m = re.search(r"typedef struct azh_access \{(.*?)\} azh_access;", hdr, flags=re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [f.strip() for decl in body.split(";") if decl.strip() for f in decl.split(None, 1)[1].split(",")]
    assert fields == list(native.ACCESS_DTYPE.names)

    class Access(C.Structure):  # the header's declaration, laid out by the C rules
        _fields_ = [("t_start_min", C.c_double), ("t_end_min", C.c_double), ("min_range_km", C.c_double), ("flags", C.c_uint32),
                    ("grid_start", C.c_uint32), ("grid_end", C.c_uint32), ("grid_min_range", C.c_uint32)]
    assert C.sizeof(Access) == 40 and native.ACCESS_DTYPE.itemsize == 40
    want = {"t_start_min": 0, "t_end_min": 8, "min_range_km": 16, "flags": 24, "grid_start": 28, "grid_end": 32, "grid_min_range": 36}
    for name, off in want.items():
        assert getattr(Access, name).offset == off and native.ACCESS_DTYPE.fields[name][1] == off, name
    for name, value in (("AZH_ACCESS_OPEN_AT_START", native.ACCESS_OPEN_AT_START), ("AZH_ACCESS_OPEN_AT_END", native.ACCESS_OPEN_AT_END),
                        ("AZH_ACCESS_CUT_BY_ERROR", native.ACCESS_CUT_BY_ERROR)):
        assert re.search(r"#define %s %du\b" % (name, value), hdr)
    assert (native.ACCESS_OPEN_AT_START, native.ACCESS_OPEN_AT_END, native.ACCESS_CUT_BY_ERROR) == (1, 2, 4)


def _pairs():
    """Pairs of positions between 6,500 and 42,164 km: random ones, and the special cases, labelled."""
    rng = np.random.default_rng(17)
    out = []
    for _ in range(4000):  # random directions and radii: all three tau regimes occur
        a, b = rng.uniform(6500.0, 42164.0, 2)
        out.append(("random", a * _unit(rng), b * _unit(rng)))
    for _ in range(500):  # nearly the same direction: the closest point of the line lies outside the segment
        u = _unit(rng)
        v = u + 0.05 * rng.normal(size=3)
        a, b = rng.uniform(6500.0, 42164.0, 2)
        out.append(("radial", a * u, b * v / np.linalg.norm(v)))
    for _ in range(500):  # side by side, from a metre to a hundred kilometres apart
        u = _unit(rng)
        a = rng.uniform(6500.0, 42164.0)
        t = np.cross(u, _unit(rng))
        out.append(("close", a * u, a * u + 10.0 ** rng.uniform(-3, 2) * t / np.linalg.norm(t) + rng.normal(size=3) * 1e-4))
    for h in (0.0, 100.0):  # a line grazing R + h within 1e-6 km on both sides
        for _ in range(200):
            u = _unit(rng)
            t = np.cross(u, _unit(rng))
            t /= np.linalg.norm(t)
            for eps in (-1e-6, -1e-9, 1e-9, 1e-6):
                foot = (R_EARTH + h + eps) * u
                out.append(("graze %g %g" % (h, eps), foot - rng.uniform(500.0, 41000.0) * t, foot + rng.uniform(500.0, 41000.0) * t))
    for _ in range(50):
        u = _unit(rng)
        a = rng.uniform(6500.0, 42164.0)
        out.append(("coincident", a * u, a * u))
        out.append(("antipodal", a * u, -a * u))
        out.append(("below", rng.uniform(5000.0, R_EARTH + 99.0) * u, a * _unit(rng)))  # one object below R + h
    return out


def test_line_of_sight_matches_extended_precision(native):
    """Clearance and range against the longdouble restatement.  The bound: the issue's "5e-12 km relative to 4.2e4 km
    operands" is taken as the relative figure 5e-12 of the larger operand (2.1e-7 km at 4.2e4 km).  It cannot be an absolute
    5e-12 km: |d| between two geostationary positions reaches 8.4e4 km, where neighbouring doubles are 1.5e-11 km apart.  The
    clear / blocked answer must be the restatement's wherever the margin exceeds that bound."""
    L = native.lib()
    seen = {"le0": 0, "inside": 0, "ge1": 0}
    worst_c = worst_r = 0.0
    cl, rg = C.c_double(), C.c_double()
    for label, r1, r2 in _pairs():
        r1, r2 = np.ascontiguousarray(r1), np.ascontiguousarray(r2)
        wc, wr, tau = longdouble_los(r1, r2)
        seen["le0" if tau <= 0 else "ge1" if tau >= 1 else "inside"] += 1
        for h in (0.0, 100.0):
            ok = L.azh_line_of_sight(r1.ctypes.data, r2.ctypes.data, h, C.addressof(cl), C.addressof(rg))
            tol = 5e-12 * max(np.linalg.norm(r1), np.linalg.norm(r2))
            ec, er = abs(cl.value - float(wc)), abs(rg.value - float(wr))
            worst_c, worst_r = max(worst_c, ec / tol), max(worst_r, er / tol)
            assert ec <= tol and er <= tol, (label, r1, r2, cl.value, float(wc), rg.value, float(wr))
            margin = float(wc) - (R_EARTH + h)
            if abs(margin) > tol:
                assert ok == (1 if margin >= 0 else 0), (label, h, margin)
            assert ok == (1 if cl.value - (R_EARTH + h) >= 0 else 0)
            assert native.line_of_sight(r1, r2, h) == (bool(ok), cl.value, rg.value)
        if label.startswith("graze"):
            h, eps = (float(x) for x in label.split()[1:])
            assert 0 < tau < 1
            if abs(eps) >= 1e-6:  # 1e-6 km is above the bound: the side is decided
                assert L.azh_line_of_sight(r1.ctypes.data, r2.ctypes.data, h, None, None) == (1 if eps > 0 else 0), (label, r1, r2)
        if label == "coincident":
            assert rg.value == 0.0 and cl.value == pytest.approx(np.linalg.norm(r1), rel=1e-15)
        if label == "antipodal":
            assert cl.value <= 5e-12 * np.linalg.norm(r1) and L.azh_line_of_sight(r1.ctypes.data, r2.ctypes.data, 0.0, None, None) == 0
        if label == "below":
            assert L.azh_line_of_sight(r1.ctypes.data, r2.ctypes.data, 100.0, None, None) == 0
    print("tau <= 0: %(le0)d, inside: %(inside)d, tau >= 1: %(ge1)d" % seen)
    print("worst error as a fraction of the bound: clearance %.3g, range %.3g" % (worst_c, worst_r))
    assert min(seen.values()) >= 300


def test_null_pointers_and_value_errors(native):
    """The paths that return before a handle or a device is touched."""
    L = native.lib()
    a, b = np.array([7000.0, 0.0, 0.0]), np.array([0.0, 7000.0, 0.0])
    assert L.azh_line_of_sight(None, b.ctypes.data, 0.0, None, None) == -1
    assert L.azh_line_of_sight(a.ctypes.data, None, 0.0, None, None) == -1
    assert L.azh_line_of_sight(a.ctypes.data, b.ctypes.data, 0.0, None, None) == 0  # the output pointers are optional
    far = a + b  # (the segment leaves a at right angles to its radius: clearance |a|)
    assert L.azh_line_of_sight(a.ctypes.data, far.ctypes.data, 0.0, None, None) == 1
    cnt = np.zeros(4, dtype=np.uint32)
    t = np.arange(4.0)
    inf = float("inf")

    def host(times=t, h=100.0, rng=inf, room=0, cnt_p=cnt.ctypes.data):
        return L.azh_find_access_host(None, times.ctypes.data, len(times), None, 0, h, rng, None, room, cnt_p, None)

    def device(times=t, h=100.0, rng=inf, room=0):
        return L.azh_find_access_device(None, times.ctypes.data, len(times), None, 0, h, rng, None, room, cnt.ctypes.data, None, None)

    def track(times=t, h=100.0, rng=inf, room=0):
        return L.azh_find_access_track_device(None, times.ctypes.data, len(times), None, t.ctypes.data, t.ctypes.data, 0, h, rng, None,
                                              room, cnt.ctypes.data, None, None)
    for call in (host, device, track):
        assert call() == NULL  # no handle
        for bad_t in (np.array([0.0, 1.0, 1.0]), np.array([2.0, 1.0]), np.array([0.0, np.nan, 2.0])):
            assert call(times=bad_t) == VALUE
        for bad_h in (-1.0, float("nan"), inf, -inf):
            assert call(h=bad_h) == VALUE
        for bad_r in (0.0, -5.0, float("nan"), -inf):
            assert call(rng=bad_r) == VALUE
        assert call(rng=5000.0) == NULL and call(h=0.0) == NULL
        assert call(room=1 << 32) == VALUE and call(room=0xffffffff) == NULL
    assert host(cnt_p=None) == NULL


def test_python_argument_checks(native, monkeypatch):
    import astroz_amd
    assert {"access", "ACCESS_DTYPE"} <= set(astroz_amd.__all__)
    assert astroz_amd.ACCESS_DTYPE.names == ("sat", "start", "end", "min_range", "t_min_range", "flags")

    def no_handle(*a, **k):
        raise AssertionError("argument errors must be raised before a constellation is built")
    monkeypatch.setattr(astroz_amd, "Constellation", no_handle)
    good = [0.0, 1.0]
    for times in ([0.0, 1.0, 1.0], [2.0, 1.0], [0.0, np.nan, 2.0], [[0.0, 1.0], [2.0, 3.0]]):
        with pytest.raises(ValueError):
            astroz_amd.access("x", times, 0)
    for target in (None, -1, 1.5, "first"):
        with pytest.raises(ValueError):
            astroz_amd.access("x", good, target)
    for h in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            astroz_amd.access("x", good, 0, grazing_altitude=h)
    for r in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            astroz_amd.access("x", good, 0, max_range=r)
