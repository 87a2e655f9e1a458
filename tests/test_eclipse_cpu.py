"""CPU tier of the eclipse finder: the host twins of the Sun model and the shadow function (pure host exports), the ABI
constants and the argument checks that need no device."""
import re

import numpy as np
import pytest

AU = 149597870.7
R_EARTH, R_SUN = 6378.137, 696000.0


def numpy_sun(jd):
    """The low-precision Almanac series (Vallado, algorithm "Sun"), written from the published formula: km."""
    jd = np.asarray(jd, dtype=np.float64)
    T = (jd - 2451545.0) / 36525.0
    lam_m = np.mod(280.460 + 36000.771 * T, 360.0)
    M = np.radians(np.mod(357.5291092 + 35999.05034 * T, 360.0))
    lam = np.radians(lam_m + 1.914666471 * np.sin(M) + 0.019994643 * np.sin(2 * M))
    r = 1.000140612 - 0.016708617 * np.cos(M) - 0.000139589 * np.cos(2 * M)
    eps = np.radians(23.439291 - 0.0130042 * T)
    return AU * np.stack([r * np.cos(lam), r * np.cos(eps) * np.sin(lam), r * np.sin(eps) * np.sin(lam)], axis=-1)


def longdouble_shadow(r, sun):
    """f_umbra, f_penumbra and the 0/1/2 state by the formulas of the model, in extended precision."""
    r, sun = np.asarray(r, dtype=np.longdouble), np.asarray(sun, dtype=np.longdouble)
    d = np.sqrt((sun * sun).sum())
    s = sun / d
    x = -(r * s).sum()
    h = np.sqrt(max((r * r).sum() - x * x, np.longdouble(0)))
    su, sp = (R_SUN - R_EARTH) / d, (R_SUN + R_EARTH) / d
    fu = h - (R_EARTH - x * su / np.sqrt(1 - su * su))
    fp = h - (R_EARTH + x * sp / np.sqrt(1 - sp * sp))
    state = 0 if x <= 0 else 2 if fu < 0 else 1 if fp < 0 else 0
    return fu, fp, state


def test_symbols_and_abi(native):
    L = native.lib()
    for name in ("azh_sun_position_teme", "azh_selftest_sun", "azh_shadow_state", "azh_find_eclipses_host",
                 "azh_find_eclipses_device"):
        assert hasattr(L, name) and name in native.EXPORTS
    hdr = open(native.os.path.join(native._HERE, "..", "include", "astroz_hip.h")).read()
    m = re.search(r"typedef struct azh_eclipse \{(.*?)\} azh_eclipse;", hdr, flags=re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [f.strip() for decl in body.split(";") if decl.strip() for f in decl.split(None, 1)[1].split(",")]
    assert fields == list(native.ECLIPSE_DTYPE.names) and native.ECLIPSE_DTYPE.itemsize == 32
    for name, value in (("AZH_ECLIPSE_IN_AT_START", native.ECLIPSE_IN_AT_START), ("AZH_ECLIPSE_IN_AT_END", native.ECLIPSE_IN_AT_END),
                        ("AZH_ECLIPSE_CUT_BY_ERROR", native.ECLIPSE_CUT_BY_ERROR)):
        assert re.search(r"#define %s %du\b" % (name, value), hdr)
    assert re.search(r"AZH_SHADOW_UMBRA = 0, AZH_SHADOW_PENUMBRA = 1", hdr)
    assert (native.SHADOW_UMBRA, native.SHADOW_PENUMBRA) == (0, 1)


def test_sun_known_answer(native):
    """Vallado's example 5-1: 2 April 2006, 00:00 -- the printed vector has seven digits; the formula was measured 1.1e-6 AU
    from it, the gate is four times that."""
    s = native.sun_position(2453827.5) / AU
    want = np.array([0.9771945, 0.1924424, 0.0834308])
    print("sun(2453827.5) = %r AU, |d| = %.3g AU" % (s.tolist(), np.abs(s - want).max()))
    assert np.abs(s - want).max() <= 5e-6


def test_sun_matches_numpy_restatement(native):
    import astroz_amd
    jd = np.linspace(2447892.5, 2469807.5, 20001)  # 1990-01-01 .. 2050-01-01
    got = astroz_amd.sun_position(jd)
    assert got.shape == (len(jd), 3)
    want = numpy_sun(jd)
    rel = np.linalg.norm(got - want, axis=1) / np.linalg.norm(want, axis=1)
    print("sun vs numpy: max relative difference %.3g" % rel.max())
    assert rel.max() <= 1e-9
    # vectorised over any shape, scalars included
    assert astroz_amd.sun_position(2453827.5).shape == (3,)
    assert astroz_amd.sun_position(jd[:6].reshape(2, 3)).shape == (2, 3, 3)
    assert np.array_equal(astroz_amd.sun_position(jd[:6].reshape(2, 3)).reshape(6, 3), got[:6])
    # distance and ecliptic geometry stay physical over the whole span
    d = np.linalg.norm(got, axis=1) / AU
    assert 0.983 < d.min() < 0.9834 and 1.0166 < d.max() < 1.0168


def _frame(sun):
    """Unit vector to the Sun and two unit vectors perpendicular to it."""
    s = sun / np.linalg.norm(sun)
    a = np.cross(s, [0.0, 0.0, 1.0])
    a /= np.linalg.norm(a)
    return s, a, np.cross(s, a)


def test_shadow_state_axis_and_mirror(native):
    sun = native.sun_position(2453827.5)
    s, a, b = _frame(sun)
    st, fu, fp = native.shadow_state(-7000.0 * s, sun)
    assert st == 2 and fu < 0 and fp < 0
    st, fu, fp = native.shadow_state(7000.0 * s, sun)
    assert st == 0  # the day side: f is negative in the mirror cone too, x decides
    assert fu < 0 and fp < 0
    # far behind the Earth, beyond the tip of the umbra (R / tan a_u = 1.38e6 km): penumbra only
    assert native.shadow_state(-1.6e6 * s, sun)[0] == 1


@pytest.mark.parametrize("jd", [2453827.5, 2460300.25, 2461573.5])
def test_shadow_state_matches_formulas(native, jd):
    sun = native.sun_position(jd)
    s, a, b = _frame(sun)
    d = np.linalg.norm(sun)
    tu = np.tan(np.arcsin((R_SUN - R_EARTH) / d))
    tp = np.tan(np.arcsin((R_SUN + R_EARTH) / d))
    assert abs(np.degrees(np.arctan(tu)) - 0.26413) < 0.005 and abs(np.degrees(np.arctan(tp)) - 0.26901) < 0.005
    seen = set()
    worst = 0.0
    for x in (7000.0, 42164.0, 300.0, -7000.0):
        for edge in (R_EARTH - x * tu, R_EARTH + x * tp):  # the umbra's and the penumbra's edge at this x
            for dh in (-1.0, -1e-3, 1e-3, 1.0):
                for axis in (a, b, (a + b) / np.sqrt(2.0)):
                    r = -x * s + (edge + dh) * axis
                    st, fu, fp = native.shadow_state(r, sun)
                    wu, wp, wst = longdouble_shadow(r, sun)
                    worst = max(worst, abs(fu - float(wu)), abs(fp - float(wp)))
                    assert abs(fu - float(wu)) <= 1e-9 and abs(fp - float(wp)) <= 1e-9, (x, dh, fu, wu, fp, wp)
                    assert (fu < 0) == (wu < 0) and (fp < 0) == (wp < 0) and st == wst, (x, dh, st, wst)
                    seen.add(st)
    print("shadow values vs long double: max difference %.3g km" % worst)
    assert seen == {0, 1, 2}


def test_null_pointers(native):
    L = native.lib()
    buf = np.zeros(8)
    assert L.azh_shadow_state(None, buf.ctypes.data, None, None) == -1
    assert L.azh_shadow_state(buf.ctypes.data, None, None, None) == -1
    L.azh_sun_position_teme(2453827.5, None)  # returns
    sun = native.sun_position(2453827.5)
    r = np.ascontiguousarray(-7000.0 * sun / np.linalg.norm(sun))
    assert L.azh_shadow_state(r.ctypes.data, sun.ctypes.data, None, None) == 2  # the f pointers are optional
    cnt = np.zeros(4, dtype=np.uint32)
    t = np.arange(4.0)
    AZ_ERR_NULL_POINTER = -101
    assert L.azh_find_eclipses_host(None, t.ctypes.data, 4, None, 2460000.5, 0, None, 0, cnt.ctypes.data, None) == AZ_ERR_NULL_POINTER
    assert L.azh_find_eclipses_device(None, t.ctypes.data, 4, None, 2460000.5, 0, None, 0, cnt.ctypes.data, None, None) == AZ_ERR_NULL_POINTER
    assert L.azh_selftest_sun(None, 4, buf.ctypes.data, 0) == AZ_ERR_NULL_POINTER


def test_python_argument_checks(native, monkeypatch):
    import astroz_amd
    assert {"eclipses", "sun_position", "ECLIPSE_DTYPE"} <= set(astroz_amd.__all__)
    assert astroz_amd.ECLIPSE_DTYPE.names == ("sat", "entry", "exit", "flags")

    def no_handle(*a, **k):
        raise AssertionError("argument errors must be raised before a constellation is built")
    monkeypatch.setattr(astroz_amd, "Constellation", no_handle)
    with pytest.raises(ValueError):
        astroz_amd.eclipses("x", [0.0, 1.0], kind="antumbra")
    for times in ([0.0, 1.0, 1.0], [2.0, 1.0], [0.0, np.nan, 2.0], [[0.0, 1.0], [2.0, 3.0]]):
        with pytest.raises(ValueError):
            astroz_amd.eclipses("x", times)
