"""Ground coverage, the parts that need no GPU: the exports of the cross-compiled library and the record layout, null-handle
checks ahead of any device work, the argument checks of astroz_amd.coverage before it builds a handle, and grid_points."""
import os
import re
import subprocess

import numpy as np
import pytest

NULL = -101
NAMES = ("azh_coverage_host", "azh_coverage_device")


def header(native):
    return open(os.path.join(native._HERE, "..", "include", "astroz_hip.h")).read()


def test_symbols_exported(native):
    L = native.lib()
    for name in NAMES:
        assert name in native.EXPORTS
        assert hasattr(L, name)
    dyn = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in dyn.splitlines() if line.strip()}
    assert set(NAMES) <= names
    hdr = header(native)
    shim = open(os.path.join(native._HERE, "..", "bindings", "zig", "astroz_hip.zig")).read()
    for name in NAMES:
        assert re.search(r"\bint32_t %s\(" % name, hdr), name
        assert re.search(r'pub extern "c" fn %s\(' % name, shim), name


def test_record_layout_matches_header(native):
    """COVERAGE_DTYPE against the struct the header declares: the same members in the same order, doubles of 8 and uint32_t
    of 4 bytes with no padding between them (the doubles come first), a size that is a multiple of 8."""
    body = re.search(r"typedef struct azh_coverage \{(.*?)\} azh_coverage;", header(native), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = []
    for ctype, names in re.findall(r"(double|uint32_t)\s+([^;]+);", body):
        members += [(n.strip(), "<f8" if ctype == "double" else "<u4") for n in names.split(",")]
    size = sum(8 if t == "<f8" else 4 for _, t in members)
    assert size % 8 == 0
    dt = native.COVERAGE_DTYPE
    assert [(n, dt[n].str) for n in dt.names] == members
    assert dt.itemsize == size == 48
    assert [dt.fields[n][1] for n in dt.names] == list(np.cumsum([0] + [8 if t == "<f8" else 4 for _, t in members[:-1]]))
    assert (native.COVERAGE_GAP_AT_START, native.COVERAGE_GAP_AT_END) == (1, 2)
    assert "#define AZH_COVERAGE_GAP_AT_START 1u" in header(native) and "#define AZH_COVERAGE_GAP_AT_END 2u" in header(native)


def test_null_handle(native):
    L = native.lib()
    t = np.arange(10.0)
    pt = np.array([[47.3, 8.5, 0.4], [0.0, 0.0, 0.0]])
    mk = np.array([10.0, 5.0])
    stats = np.zeros(2, dtype=native.COVERAGE_DTYPE)
    cnt = np.full((2, 10), 777, dtype=np.uint32)
    args = (t.ctypes.data, len(t), None, 0.0, pt.ctypes.data, mk.ctypes.data, 2)
    assert L.azh_coverage_host(None, *args, 1, stats.ctypes.data, cnt.ctypes.data) == NULL
    assert L.azh_coverage_host(None, *args, 1, stats.ctypes.data, None) == NULL
    assert L.azh_coverage_device(None, *args, 1, None, None, None) == NULL
    # a null handle is refused whatever else is given: no points, bad points, min_satellites 0
    assert L.azh_coverage_host(None, t.ctypes.data, len(t), None, 0.0, None, None, 0, 1, None, None) == NULL
    bad = np.array([[95.0, 0.0, 0.0]])
    assert L.azh_coverage_device(None, t.ctypes.data, len(t), None, 0.0, bad.ctypes.data, mk.ctypes.data, 1, 1, stats.ctypes.data,
                                 None, None) == NULL
    assert L.azh_coverage_host(None, *args, 0, stats.ctypes.data, cnt.ctypes.data) == NULL
    assert (cnt == 777).all() and not stats.view(np.uint8).any()


class _Touched(Exception):
    pass


@pytest.fixture
def no_handles(monkeypatch):
    """coverage must reject bad input before it builds a Constellation (and so before any device work)."""
    import astroz_amd

    class Refuse:
        def __init__(self, *a, **k):
            raise _Touched()
    monkeypatch.setattr(astroz_amd, "Constellation", Refuse)
    return astroz_amd


@pytest.mark.parametrize("points", [
    [(91.0, 0.0, 0.0)], [(-90.5, 0.0, 0.0)], [(np.nan, 0.0, 0.0)], [(0.0, np.inf, 0.0)], [(0.0, 0.0, np.nan)],
    [(1.0, 2.0)], [(1.0, 2.0, 3.0, 4.0)], [("a", 0.0, 0.0)], 5.0, [(10.0, 20.0, 0.0), (1.0,)],
])
def test_bad_points(no_handles, points):
    with pytest.raises(ValueError):
        no_handles.coverage("unused", [0.0, 1.0], points)


@pytest.mark.parametrize("mask", [[10.0], [10.0, 5.0, 0.0], [[10.0, 5.0]], [10.0, np.nan], np.inf])
def test_bad_masks(no_handles, mask):
    with pytest.raises(ValueError):
        no_handles.coverage("unused", [0.0, 1.0], [(10.0, 20.0, 0.0), (-5.0, 30.0, 1.0)], min_elevation=mask)


@pytest.mark.parametrize("times", [[0.0, 1.0, 1.0], [2.0, 1.0], [0.0, np.nan, 2.0], [[0.0, 1.0], [2.0, 3.0]]])
def test_bad_times(no_handles, times):
    with pytest.raises(ValueError):
        no_handles.coverage("unused", times, [(10.0, 20.0, 0.0)])


@pytest.mark.parametrize("k", [0, -1, 1.5, 2.0, "2", None, True, 1 << 32])
def test_bad_min_satellites(no_handles, k):
    with pytest.raises(ValueError):
        no_handles.coverage("unused", [0.0, 1.0], [(10.0, 20.0, 0.0)], min_satellites=k)


def test_good_arguments_reach_the_handle(no_handles):
    # (the checks above fail for their own reason: well-formed input gets as far as building the handle)
    with pytest.raises(_Touched):
        no_handles.coverage("unused", [0.0, 1.0], [(10.0, 20.0, 0.0), (90.0, -180.0, 4.0)], min_elevation=[0.0, 30.0])
    with pytest.raises(_Touched):
        no_handles.coverage("unused", [0.0], np.array([[10.0, 20.0, 0.0]]), min_elevation=5, min_satellites=np.int64(3), counts=True)
    with pytest.raises(_Touched):
        no_handles.coverage("unused", [0.0, 1.0], no_handles.grid_points(30))


def test_public_surface(native):
    import astroz_amd
    assert {"coverage", "grid_points", "COVERAGE_DTYPE"} <= set(astroz_amd.__all__)
    assert astroz_amd.COVERAGE_DTYPE.names == ("covered_fraction", "mean_in_view", "min_in_view", "max_in_view", "n_gaps",
                                               "max_gap", "gap_start", "gap_end", "flags")


def test_grid_points():
    import astroz_amd
    g = astroz_amd.grid_points(5)
    assert g.shape == (2592, 3) and g.dtype == np.float64
    lat, lon = g[:, 0].reshape(36, 72), g[:, 1].reshape(36, 72)
    assert np.array_equal(lat[:, 0], np.arange(-87.5, 90.0, 5.0)) and (lat == lat[:, :1]).all()
    assert np.array_equal(lon[0], np.arange(-177.5, 180.0, 5.0)) and (lon == lon[:1]).all()
    assert not g[:, 2].any()
    # rectangular cells, an altitude
    g = astroz_amd.grid_points(30, 90, alt_km=1.5)
    assert g.shape == (6 * 4, 3) and (g[:, 2] == 1.5).all()
    assert np.array_equal(np.unique(g[:, 0]), [-75.0, -45.0, -15.0, 15.0, 45.0, 75.0])
    assert np.array_equal(np.unique(g[:, 1]), [-135.0, -45.0, 45.0, 135.0])
    # a latitude band; a range beyond the poles is clipped to them; the last band is cut at the upper edge
    g = astroz_amd.grid_points(10, 60, lat_range=(-20, 20))
    assert np.array_equal(np.unique(g[:, 0]), [-15.0, -5.0, 5.0, 15.0]) and len(g) == 4 * 6
    assert np.array_equal(astroz_amd.grid_points(5, lat_range=(-100, 95)), astroz_amd.grid_points(5))
    g = astroz_amd.grid_points(20, 180, lat_range=(0, 50))
    assert np.array_equal(np.unique(g[:, 0]), [10.0, 30.0, 45.0])
    # every point is one coverage() accepts
    assert (np.abs(astroz_amd.grid_points(7, 11)[:, 0]) < 90.0).all() and (np.abs(astroz_amd.grid_points(7, 11)[:, 1]) < 180.0).all()
    for bad in ((0,), (-5,), (5, 0), (5, 400), (np.nan,)):
        with pytest.raises(ValueError):
            astroz_amd.grid_points(*bad)
    with pytest.raises(ValueError):
        astroz_amd.grid_points(5, lat_range=(10, 10))
