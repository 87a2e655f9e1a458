"""Passes over several ground stations, the parts that need no GPU: the exports of the cross-compiled library, null-pointer
checks ahead of any device work, and the argument checks of astroz_amd.station_passes before it builds a handle."""
import subprocess

import numpy as np
import pytest

NULL = -101


def test_symbols_exported(native):
    L = native.lib()
    for name in ("azh_find_passes_stations_host", "azh_find_passes_stations_device"):
        assert name in native.EXPORTS
        assert hasattr(L, name)
    dyn = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in dyn.splitlines() if line.strip()}
    assert {"azh_find_passes_stations_host", "azh_find_passes_stations_device"} <= names


def test_null_pointers(native):
    L = native.lib()
    t = np.arange(10.0)
    st = np.array([[47.3, 8.5, 0.4], [0.0, 0.0, 0.0]])
    mk = np.array([10.0, 5.0])
    out = np.zeros(8, dtype=native.PASS_DTYPE)
    n = np.zeros(2, dtype=np.uint32)
    args = (t.ctypes.data, len(t), None, 0.0, st.ctypes.data, mk.ctypes.data, 2)
    assert L.azh_find_passes_stations_host(None, *args, out.ctypes.data, 4, n.ctypes.data) == NULL
    assert L.azh_find_passes_stations_device(None, *args, None, 4, None, None) == NULL
    # a null handle is refused whatever else is given, no stations and bad stations included
    assert L.azh_find_passes_stations_host(None, t.ctypes.data, len(t), None, 0.0, None, None, 0, None, 0, n.ctypes.data) == NULL
    bad = np.array([[95.0, 0.0, 0.0]])
    assert L.azh_find_passes_stations_device(None, t.ctypes.data, len(t), None, 0.0, bad.ctypes.data, mk.ctypes.data, 1, None, 0,
                                             n.ctypes.data, None) == NULL


class _Touched(Exception):
    pass


@pytest.fixture
def no_handles(monkeypatch):
    """station_passes must reject bad input before it builds a Constellation (and so before any device work)."""
    import astroz_amd

    class Refuse:
        def __init__(self, *a, **k):
            raise _Touched()
    monkeypatch.setattr(astroz_amd, "Constellation", Refuse)
    return astroz_amd


@pytest.mark.parametrize("stations", [
    [(91.0, 0.0, 0.0)], [(-90.5, 0.0, 0.0)], [(np.nan, 0.0, 0.0)], [(0.0, np.inf, 0.0)], [(0.0, 0.0, np.nan)],
    [(1.0, 2.0)], [(1.0, 2.0, 3.0, 4.0)], [("a", 0.0, 0.0)], 5.0, [(10.0, 20.0, 0.0), (1.0,)],
])
def test_bad_stations(no_handles, stations):
    with pytest.raises(ValueError):
        no_handles.station_passes("unused", [0.0, 1.0], stations)


@pytest.mark.parametrize("mask", [[10.0], [10.0, 5.0, 0.0], [[10.0, 5.0]], [10.0, np.nan], np.inf])
def test_bad_masks(no_handles, mask):
    with pytest.raises(ValueError):
        no_handles.station_passes("unused", [0.0, 1.0], [(10.0, 20.0, 0.0), (-5.0, 30.0, 1.0)], min_elevation=mask)


@pytest.mark.parametrize("times", [[0.0, 1.0, 1.0], [2.0, 1.0], [0.0, np.nan, 2.0], [[0.0, 1.0], [2.0, 3.0]]])
def test_bad_times(no_handles, times):
    with pytest.raises(ValueError):
        no_handles.station_passes("unused", times, [(10.0, 20.0, 0.0)])


def test_good_arguments_reach_the_handle(no_handles):
    # (the checks above fail for their own reason: well-formed input gets as far as building the handle)
    with pytest.raises(_Touched):
        no_handles.station_passes("unused", [0.0, 1.0], [(10.0, 20.0, 0.0), (90.0, -180.0, 4.0)], min_elevation=[0.0, 30.0])
    with pytest.raises(_Touched):
        no_handles.station_passes("unused", [0.0], np.array([[10.0, 20.0, 0.0]]), min_elevation=5)


def test_public_surface(native):
    import astroz_amd
    assert "station_passes" in astroz_amd.__all__
    assert astroz_amd.STATION_PASS_DTYPE.names == ("station", "sat", "rise", "culmination", "set", "max_elevation",
                                                   "rise_azimuth", "set_azimuth", "flags")
    assert astroz_amd.STATION_PASS_DTYPE["station"] == np.dtype("<u4")
    hdr = open(native.os.path.join(native._HERE, "..", "include", "astroz_hip.h")).read()
    assert "azh_find_passes_stations_host" in hdr and "azh_find_passes_stations_device" in hdr
