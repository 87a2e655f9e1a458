"""astroz_amd -- MI355X-native batched SGP4/SDP4 constellation propagation.

Drop-in for the batched-propagation path of ATTron/astroz's Python package: :class:`Constellation`,
:func:`propagate`, :func:`screen` (bindings/python/astroz/__init__.py L305-658) and the extension type
:class:`Sgp4Constellation` (bindings/python/astroz/_astroz.pyi L501-630) with the same arguments, shapes and
defaults; the python-sgp4 compatible layer is :mod:`astroz_amd.api`.  All arithmetic runs in hand-written
gfx950 HIP kernels behind ``libastroz_hip.so`` (C ABI in ``include/astroz_hip.h``); there is no CPU fallback.

Element text goes to the library as it is: TLE text is read by the library's fixed-column reader, OMM JSON by
its OMM reader (full JSON precision; the reference's Python layer re-renders OMM as 69-column text first and
loses digits there).

Network sources are OPT-IN.  Like the reference, ``source`` may also be a URL or a CelesTrak group name and
``norad_id=`` a catalog number (or a list), but nothing is downloaded unless the caller allows it: pass
``fetch=callable(url) -> str`` (or install one with :func:`set_fetcher`), or ``allow_network=True`` to use the
built-in ``urllib`` fetcher.  Without either such a source raises ``ValueError`` naming the URL it would have
fetched.  The fetched text goes to the same native readers as any other text.
"""
import os
from datetime import datetime, timezone

import numpy as np

from . import _native
from ._native import WGS72, WGS84  # noqa: F401

__version__ = "0.2.0"

_UNIX_EPOCH_JD = 2440587.5


_CELESTRAK_GP = "https://celestrak.org/NORAD/elements/gp.php"
# group aliases of the reference's loader (bindings/python/astroz/__init__.py L131-136): short names -> CelesTrak GROUP values
_GROUP_ALIASES = {"all": "active", "iss": "stations", "gps": "gps-ops", "glonass": "glo-ops"}
_fetcher = None


def set_fetcher(fn):
    """Install the process-wide fetcher used for URL / CelesTrak-group / ``norad_id`` sources: ``fn(url) -> str``
    (``None`` removes it).  Returns the previous one."""
    global _fetcher
    prev, _fetcher = _fetcher, fn
    return prev


def celestrak_url(group=None, norad_id=None, fmt="tle"):
    """The CelesTrak GP query for a group name (``"starlink"``, ``"active"``, ...) or catalog number(s)."""
    if (group is None) == (norad_id is None):
        raise ValueError("exactly one of group / norad_id")
    if norad_id is not None:
        ids = norad_id if isinstance(norad_id, (list, tuple)) else [norad_id]
        return "%s?CATNR=%s&FORMAT=%s" % (_CELESTRAK_GP, ",".join(str(int(i)) for i in ids), fmt)
    name = str(group).strip().lower()
    return "%s?GROUP=%s&FORMAT=%s" % (_CELESTRAK_GP, _GROUP_ALIASES.get(name, name), fmt)


def _urllib_fetch(url):
    import urllib.request
    req = urllib.request.Request(url, headers={"User-Agent": "astroz_amd/%s" % __version__})
    with urllib.request.urlopen(req, timeout=60) as resp:
        return resp.read().decode("utf-8")


def _download(url, fetch, allow_network):
    fn = fetch or _fetcher or (_urllib_fetch if allow_network else None)
    if fn is None:
        raise ValueError("this source needs a download (%s): pass fetch=callable(url) -> str, install one with "
                         "astroz_amd.set_fetcher, or pass allow_network=True" % url)
    text = fn(url)
    if not isinstance(text, str) or not text.strip():
        raise ValueError("the fetcher returned no element text for %s" % url)
    return text


def _as_text(source, norad_id=None, fetch=None, allow_network=False):
    """The element text behind `source`: the string itself when it already is element data, the contents of the
    local file it names, or -- opt-in, see the module docstring -- what a URL / CelesTrak group name / `norad_id`
    resolves to (reference: bindings/python/astroz/__init__.py L163-181)."""
    if norad_id is not None:   # (with both given the catalog number wins, as in the reference: __init__.py L163-166)
        return _download(celestrak_url(norad_id=norad_id), fetch, allow_network)
    if source is None:
        raise ValueError("Must specify 'source' or 'norad_id'")
    if not isinstance(source, str):
        raise TypeError("source must be a string: TLE text, OMM JSON text, a local file path, a URL or a CelesTrak group")
    head = source.lstrip()[:1]
    if head in ("{", "["):
        return source
    one_line = "\n" not in source and len(source) < 4096
    if one_line and source.lower().startswith(("http://", "https://")):
        if source.lower().startswith("http://"):
            import warnings
            warnings.warn("element sets fetched over plain http are not authenticated: prefer https", stacklevel=3)
        return _download(source, fetch, allow_network)
    if one_line and os.path.isfile(source):
        with open(source, "r", encoding="utf-8") as fh:
            return fh.read()
    if any(ln.lstrip().startswith("1 ") for ln in source.splitlines()):
        return source
    name = source.strip()
    if name.lower().startswith("celestrak:"):
        name = name[len("celestrak:"):].strip()   # explicit form: never mistaken for a mistyped file name
        if not name:
            raise ValueError("empty CelesTrak group name")
        return _download(celestrak_url(group=name), fetch, allow_network)
    if one_line and name and all(c.isalnum() or c in "-_" for c in name):
        return _download(celestrak_url(group=name), fetch, allow_network)
    if one_line and name and " " not in name and ("." in name or os.sep in name):
        raise FileNotFoundError(name)   # looks like a path (catalog.tle, data/active.txt) and is not there: not a group name
    raise ValueError("source is neither TLE text, OMM JSON, an existing local file, a URL nor a CelesTrak group name")


def _is_json(text):
    return text.lstrip()[:1] in ("{", "[")


def _jd_of(start_time):
    """Julian date of a datetime; None means now (UTC)."""
    when = datetime.now(timezone.utc) if start_time is None else start_time
    return _UNIX_EPOCH_JD + when.timestamp() / 86400.0


class Tle:
    """Two-Line Element set: ``astroz.Tle(tle_string)`` (bindings/python/src/tle.zig L14-104) over the
    c_api ``tle_parse`` / ``tle_get_*`` exports.  Text parsing only -- no GPU involved."""

    def __init__(self, tle_string):
        import ctypes as C
        if not isinstance(tle_string, str):
            raise TypeError("tle_string must be str")
        h = C.c_void_p()
        if _native.lib().tle_parse(tle_string.encode(), C.byref(h)) != 0:
            raise ValueError("Failed to parse TLE")
        self._h = h

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            _native.lib().tle_free(h)
            self._h = None

    satellite_number = property(lambda self: int(_native.lib().tle_get_satellite_number(self._h)),
                                doc="NORAD catalog number")
    epoch = property(lambda self: float(_native.lib().tle_get_epoch(self._h)), doc="Epoch (J2000 seconds)")
    inclination = property(lambda self: float(_native.lib().tle_get_inclination(self._h)), doc="Inclination (degrees)")
    eccentricity = property(lambda self: float(_native.lib().tle_get_eccentricity(self._h)), doc="Eccentricity")
    mean_motion = property(lambda self: float(_native.lib().tle_get_mean_motion(self._h)), doc="Mean motion (rev/day)")


class Sgp4Constellation:
    """``_astroz.Sgp4Constellation`` (bindings/python/astroz/_astroz.pyi L501-630): the extension type behind the
    reference's high-level functions, same method names and keywords, device-resident elements.

    Differences that are deliberate: deep-space members are accepted and propagated (the reference's type
    rejects them); ``satellite_mask`` may be bool or uint8."""

    def __init__(self, dev):
        self._dev = dev

    @staticmethod
    def from_tle_text(tle_text, gravity_model=WGS84, device=0):
        """WGS84 is the reference's default for this constructor (bindings/python/src/sgp4.zig L293-300)."""
        return Sgp4Constellation(_native.DeviceConstellation.from_tle_text(tle_text, gravity_model, device))

    @staticmethod
    def from_omm_json(json_text, gravity_model=WGS84, device=0):
        return Sgp4Constellation(_native.DeviceConstellation.from_omm_json(json_text, gravity_model, device))

    @property
    def num_satellites(self):
        return int(self._dev.n)

    @property
    def epochs(self):
        return [float(x) for x in self._dev.epochs]

    def propagate_into(self, times, positions, velocities=None, *, epoch_offsets=None, satellite_mask=None,
                       output="ecef", reference_jd=0.0, time_major=True, output_stride=-1, observer=None):
        """Propagate into caller-owned arrays (sgp4.zig L170-262): ``(n_times, stride, 3)`` if `time_major`
        else ``(n_sats, n_times, 3)``; ``output_stride`` > 0 overrides the row length of the time-major
        layout; raises ValueError when an array is too small.  ``output="topocentric"`` needs
        ``observer=(lat_deg, lon_deg, alt_km)`` (see :func:`propagate`)."""
        _check_output(output, observer)
        if observer is not None:
            self._dev.set_observer(*_observer3(observer))
        mask = None if satellite_mask is None else np.ascontiguousarray(satellite_mask).astype(np.uint8)
        self._dev.propagate_host(times, epoch_offsets, pos=positions, vel=velocities,
                                 mode=_native.OUTPUT_MODES[output], reference_jd=float(reference_jd), mask=mask,
                                 layout=_native.TIME_MAJOR if time_major else _native.SAT_MAJOR,
                                 stride=int(output_stride) if output_stride and output_stride > 0 else 0)

    def screen_conjunction(self, times, target, threshold, *, epoch_offsets=None, reference_jd=0.0):
        """Fused propagate + single-target screen: ``(min_distances, min_t_indices)`` as lists."""
        d, ti = self._dev.screen_target(times, int(target), float(threshold), epoch_offsets, reference_jd=reference_jd)
        return [float(x) for x in d], [int(x) for x in ti]


class Constellation:
    """Pre-parsed, device-resident orbital elements for repeated propagation and screening.

    ``source``: raw TLE text, raw OMM JSON (object or array), a local file holding either, or -- with ``fetch=`` /
    ``allow_network=True`` / :func:`set_fetcher` -- a URL or CelesTrak group name; ``norad_id=`` likewise.
    Output ordering follows the reference: near-earth satellites first ``[0, n_sgp4)``, deep-space after
    (reference __init__.py L374-393) -- but the deep-space rows ARE propagated here (the reference leaves them
    unwritten, L509-530).  The gravity model is WGS84, the default of the reference's ``from_tle_text``."""

    def __init__(self, source=None, *, norad_id=None, gravity_model=WGS84, device=0, fetch=None, allow_network=False):
        text = _as_text(source, norad_id, fetch, allow_network)
        build = _native.DeviceConstellation.from_omm_json if _is_json(text) else _native.DeviceConstellation.from_tle_text
        try:
            full = build(text, gravity_model, device)
        except _native.NativeError as exc:
            if exc.code == _native.AZ_ERR_HIP:
                raise
            raise ValueError("no usable element sets found in source") from exc
        err, deep, _ = full.status
        if err.any():
            bad = int(np.flatnonzero(err)[0])
            raise ValueError("%s (record %d)" % ("Invalid eccentricity" if err[bad] == 1 else "Satellite decayed", bad))
        # catalog index of every output row: near-earth members first, deep-space members after
        self._catalog_index = np.concatenate([np.flatnonzero(~deep), np.flatnonzero(deep)]).astype(np.uint32)
        if np.array_equal(self._catalog_index, np.arange(full.n, dtype=np.uint32)):
            self._dev = full
        else:
            self._dev = full.subset(self._catalog_index)  # device-side re-order: no second parse
            full.close()
        self._n_sgp4 = int((~deep).sum())
        self._total_sats = int(self._dev.n)

    @property
    def num_satellites(self):
        return self._total_sats

    @property
    def epochs(self):
        """TLE epoch of each satellite (output order) as a Julian date."""
        return [float(x) for x in self._dev.epochs]

    @property
    def catalog_index(self):
        """Position in the source text of every output row (near-earth first reorders mixed catalogs)."""
        return self._catalog_index.copy()


_OUTPUT_ERROR = "output must be 'ecef', 'teme', 'geodetic' or 'topocentric'"


def _observer3(observer):
    try:
        lat, lon, alt = (float(x) for x in observer)
    except (TypeError, ValueError):
        raise ValueError("observer must be (lat_deg, lon_deg, alt_km)") from None
    if not (np.isfinite([lat, lon, alt]).all() and abs(lat) <= 90.0):
        raise ValueError("observer must be finite with |lat_deg| <= 90")
    return lat, lon, alt


def _check_output(output, observer):
    if output not in _native.OUTPUT_MODES:
        raise ValueError(_OUTPUT_ERROR)
    if output == "topocentric" and observer is None:
        raise ValueError("output='topocentric' needs observer=(lat_deg, lon_deg, alt_km)")
    if output != "topocentric" and observer is not None:
        raise ValueError("observer= applies to output='topocentric' only")


def _minutes_and_offsets(const, times, start_time):
    minutes = np.ascontiguousarray(times, dtype=np.float64)
    start = _jd_of(start_time)
    return minutes, (start - const._dev.epochs) * 1440.0, start


def propagate(source, times, *, start_time=None, output="ecef", velocities=False, norad_id=None, fetch=None,
              allow_network=False, observer=None):
    """Propagate satellites to ``times`` (minutes from ``start_time``, default now).

    Returns positions ``(n_times, n_satellites, 3)`` [km; or (lat rad, lon rad, alt km) for
    ``output="geodetic"`` -- radians, as the reference's kernel emits (Constellation.zig L497)], plus
    velocities ``(n_times, n_satellites, 3)`` km/s if ``velocities=True``.  Reference: __init__.py L411-532.

    ``output="topocentric"`` with ``observer=(lat_deg, lon_deg, alt_km)`` (geodetic WGS84): look angles from the observer,
    (azimuth rad from north toward east in [0, 2 pi), elevation rad, range km), and with ``velocities=True`` their rates
    (rad/s, rad/s, km/s) -- the range rate is that of the Earth-fixed relative velocity (Doppler)."""
    const = source if isinstance(source, Constellation) else Constellation(source, norad_id=norad_id, fetch=fetch,
                                                                           allow_network=allow_network)
    _check_output(output, observer)
    if observer is not None:
        const._dev.set_observer(*_observer3(observer))
    minutes, offsets, start = _minutes_and_offsets(const, times, start_time)
    shape = (len(minutes), const.num_satellites, 3)
    pos = _native.result_empty(shape)     # (large results: pinned memory the device-to-host DMA writes directly)
    vel = _native.result_empty(shape) if velocities else None
    const._dev.propagate_host(minutes, offsets, pos=pos, vel=vel, mode=_native.OUTPUT_MODES[output],
                              reference_jd=start, layout=_native.TIME_MAJOR)
    return (pos, vel) if velocities else pos


def passes(source, times, observer, *, min_elevation=10.0, start_time=None, norad_id=None, fetch=None, allow_network=False):
    """Passes of every satellite over a ground station during ``times`` (minutes from ``start_time``, default now; strictly
    increasing).  ``observer=(lat_deg, lon_deg, alt_km)`` geodetic WGS84; ``min_elevation`` in degrees.

    Returns a numpy structured array, one row per pass, sorted by (sat, rise): ``sat`` (output row), ``rise``,
    ``culmination``, ``set`` (minutes from ``start_time``, refined between grid points by cubic Hermite interpolation of the
    elevation and its rate), ``max_elevation``, ``rise_azimuth``, ``set_azimuth`` (rad) and ``flags`` (1: already up at the
    first time, 2: still up at the last, 4: cut by a failed propagation; an open end is the grid time).  The propagation and
    the search run on the GPU; only the pass records come back."""
    lat, lon, alt = _observer3(observer)
    const = source if isinstance(source, Constellation) else Constellation(source, norad_id=norad_id, fetch=fetch,
                                                                           allow_network=allow_network)
    minutes, offsets, start = _minutes_and_offsets(const, times, start_time)
    if len(minutes) > 1 and not (np.diff(minutes) > 0).all():
        raise ValueError("times must be strictly increasing")
    const._dev.set_observer(lat, lon, alt)
    rec, cnt = const._dev.find_passes(minutes, offsets, reference_jd=start, min_elevation_deg=float(min_elevation), max_passes=16)
    if cnt.size and int(cnt.max()) > rec.shape[1]:  # more passes than room: once more with room for all of them
        rec, cnt = const._dev.find_passes(minutes, offsets, reference_jd=start, min_elevation_deg=float(min_elevation),
                                          max_passes=int(cnt.max()))
    idx, out = _pass_rows(rec, cnt, PASS_DTYPE)
    out["sat"] = idx
    return out


def _pass_rows(rec, cnt, dtype):
    """The passes of records ``rec`` (rows, max_passes) with counts ``cnt`` (rows,), one per row of a new ``dtype`` array in
    (row, k) order with the ``PASS_DTYPE`` fields filled, and the row index of each."""
    idx = np.repeat(np.arange(len(cnt), dtype=np.intp), cnt)
    k = np.concatenate([np.arange(c, dtype=np.intp) for c in cnt]) if len(cnt) else np.zeros(0, dtype=np.intp)
    r = rec[idx, k] if len(idx) else rec.reshape(-1)[:0]
    out = np.empty(len(idx), dtype=dtype)
    out["rise"], out["culmination"], out["set"] = r["t_rise_min"], r["t_culm_min"], r["t_set_min"]
    out["max_elevation"], out["rise_azimuth"], out["set_azimuth"] = r["max_elevation_rad"], r["rise_azimuth_rad"], r["set_azimuth_rad"]
    out["flags"] = r["flags"]
    return idx, out


# passes(): one row per pass
PASS_DTYPE = np.dtype([("sat", "<u4"), ("rise", "<f8"), ("culmination", "<f8"), ("set", "<f8"), ("max_elevation", "<f8"),
                       ("rise_azimuth", "<f8"), ("set_azimuth", "<f8"), ("flags", "<u4")])
# station_passes(): one row per pass, with its station
STATION_PASS_DTYPE = np.dtype([("station", "<u4")] + PASS_DTYPE.descr)
# the records station_passes() asks one C call for (the stations are split over several calls beyond it; each repropagates)
_STATION_CALL_BYTES = 256 << 20


def _stations_and_masks(stations, min_elevation):
    """``stations`` as an (S, 3) float64 array and ``min_elevation`` as its (S,) masks, or ValueError."""
    try:
        st = np.array([[float(x) for x in s] for s in stations], dtype=np.float64)
    except (TypeError, ValueError):
        st = None
    if st is None or (st.size and (st.ndim != 2 or st.shape[1] != 3)):
        raise ValueError("stations must be a sequence of (lat_deg, lon_deg, alt_km)")
    st = st.reshape(-1, 3)
    if not (np.isfinite(st).all() and (np.abs(st[:, 0]) <= 90.0).all()):
        raise ValueError("stations must be finite with |lat_deg| <= 90")
    mask = np.asarray(min_elevation, dtype=np.float64)
    if mask.ndim == 0:
        mask = np.full(len(st), float(mask))
    if mask.shape != (len(st),):
        raise ValueError("min_elevation must be a scalar or one value per station")
    if not np.isfinite(mask).all():
        raise ValueError("min_elevation must be finite")
    return st, mask


def _increasing_minutes(times):
    """``times`` as a 1-D float64 array, strictly increasing, or ValueError."""
    minutes = np.ascontiguousarray(times, dtype=np.float64)
    if minutes.ndim != 1 or (len(minutes) > 1 and not (np.diff(minutes) > 0).all()):
        raise ValueError("times must be strictly increasing")
    return minutes


def station_passes(source, times, stations, *, min_elevation=10.0, start_time=None, norad_id=None, fetch=None,
                   allow_network=False):
    """Passes of every satellite over each of several ground stations, from one propagation of the catalog.

    ``stations``: a sequence of ``(lat_deg, lon_deg, alt_km)`` (geodetic WGS84); ``min_elevation``: degrees, a scalar or one
    value per station; ``times`` as for ``passes()`` (strictly increasing).  Returns a numpy structured array, one row per
    pass, sorted by (station, sat, rise): ``station`` (index into ``stations``) and the fields of ``passes()``.  Station st's
    rows are the passes ``passes(source, times, stations[st], min_elevation=...)`` finds (times and angles equal to within
    the last bits); the constellation's own observer is not changed."""
    st, mask = _stations_and_masks(stations, min_elevation)
    minutes = _increasing_minutes(times)
    const = source if isinstance(source, Constellation) else Constellation(source, norad_id=norad_id, fetch=fetch,
                                                                           allow_network=allow_network)
    minutes, offsets, start = _minutes_and_offsets(const, minutes, start_time)
    n = const.num_satellites
    parts = []
    room = 16
    lo = 0
    while lo < len(st):
        # stations per call: their records within _STATION_CALL_BYTES
        k = max(1, min(len(st) - lo, _STATION_CALL_BYTES // max(1, n * room * _native.PASS_DTYPE.itemsize)))
        rec, cnt = const._dev.find_passes_stations(minutes, offsets, st[lo:lo + k], mask[lo:lo + k], reference_jd=start,
                                                   max_passes=room)
        if cnt.size and int(cnt.max()) > room:  # more passes than room: these stations once more with room for all of them
            room = int(cnt.max())
            k = max(1, min(k, _STATION_CALL_BYTES // max(1, n * room * _native.PASS_DTYPE.itemsize)))
            rec, cnt = const._dev.find_passes_stations(minutes, offsets, st[lo:lo + k], mask[lo:lo + k], reference_jd=start,
                                                       max_passes=room)
        idx, out = _pass_rows(rec.reshape(-1, rec.shape[2]), cnt.reshape(-1), STATION_PASS_DTYPE)
        out["station"] = lo + idx // max(1, n)
        out["sat"] = idx % max(1, n)
        parts.append(out)
        lo += k
    return np.concatenate(parts) if parts else np.empty(0, dtype=STATION_PASS_DTYPE)


# coverage(): one row per ground point
COVERAGE_DTYPE = np.dtype([("covered_fraction", "<f8"), ("mean_in_view", "<f8"), ("min_in_view", "<u4"), ("max_in_view", "<u4"),
                           ("n_gaps", "<u4"), ("max_gap", "<f8"), ("gap_start", "<f8"), ("gap_end", "<f8"), ("flags", "<u4")])
# the counts matrix coverage() asks one C call for (the points are split over several calls beyond it; each repropagates)
_COVERAGE_CALL_BYTES = 256 << 20


def coverage(source, times, points, *, min_elevation=10.0, min_satellites=1, start_time=None, counts=False, norad_id=None,
             fetch=None, allow_network=False):
    """Ground coverage: how many satellites each of several ground points has in view at each of ``times``, and what that
    means for the point over the whole grid.

    ``points``: a sequence of ``(lat_deg, lon_deg, alt_km)`` (geodetic WGS84; ``grid_points()`` makes a lattice);
    ``min_elevation``: degrees, a scalar or one value per point; ``times`` as for ``station_passes()`` (strictly increasing);
    ``min_satellites``: the satellites in view from which a point counts as covered.  A satellite is in view at a grid time
    when ``station_passes()`` has a pass of it over the point that holds that grid time: nothing is refined between grid
    times.  Returns a numpy structured array, one row per point: ``covered_fraction`` (covered grid times / all grid times),
    ``mean_in_view``, ``min_in_view``, ``max_in_view``, ``n_gaps`` (maximal runs of uncovered grid times), ``max_gap``
    (minutes: the longest time the point can have been uncovered, from the last covered grid time before the gap to the
    first after it, or to the ends of the grid), ``gap_start`` and ``gap_end`` (those two grid times, minutes) and ``flags``
    (1: that gap is open at the first time, 2: at the last).  With ``counts=True`` also the ``(n_points, n_times)`` uint32
    matrix of satellites in view.  The catalog is propagated and tested against every point on the GPU; only these come
    back."""
    pt, mask = _stations_and_masks(points, min_elevation)
    minutes = _increasing_minutes(times)
    k = _native._min_satellites(min_satellites)
    const = source if isinstance(source, Constellation) else Constellation(source, norad_id=norad_id, fetch=fetch,
                                                                           allow_network=allow_network)
    minutes, offsets, start = _minutes_and_offsets(const, minutes, start_time)
    n_t = len(minutes)
    out = np.zeros(len(pt), dtype=COVERAGE_DTYPE)
    matrix = np.zeros((len(pt), n_t), dtype=np.uint32) if counts else None
    per_call = max(1, _COVERAGE_CALL_BYTES // max(1, 4 * n_t))  # points per call: their counts within _COVERAGE_CALL_BYTES
    for lo in range(0, len(pt), per_call):
        hi = min(len(pt), lo + per_call)
        got = const._dev.coverage(minutes, offsets, pt[lo:hi], mask[lo:hi], reference_jd=start, min_satellites=k, counts=counts)
        st = got[0] if counts else got
        if counts:
            matrix[lo:hi] = got[1]
        o = out[lo:hi]
        o["covered_fraction"] = st["n_covered"] / float(n_t) if n_t else 0.0
        for f in ("mean_in_view", "min_in_view", "max_in_view", "n_gaps", "flags"):
            o[f] = st[f]
        o["max_gap"] = st["max_gap_min"]
        if n_t:  # the grid times that bracket the gap (its own ends where it is open)
            gap = st["n_gaps"] > 0
            o["gap_start"] = np.where(gap, minutes[np.maximum(st["grid_gap_start"].astype(np.int64) - 1, 0)], 0.0)
            o["gap_end"] = np.where(gap, minutes[np.minimum(st["grid_gap_end"].astype(np.int64) + 1, n_t - 1)], 0.0)
    return (out, matrix) if counts else out


def grid_points(lat_step_deg, lon_step_deg=None, *, lat_range=(-90, 90), alt_km=0.0):
    """The cell centres of a latitude / longitude lattice as ``(P, 3)`` points ``(lat_deg, lon_deg, alt_km)`` for
    ``coverage()``: cells of ``lat_step_deg`` x ``lon_step_deg`` (default: square) tile latitudes ``lat_range`` (clipped to
    [-90, 90]; the last band is cut at its upper edge) and longitudes [-180, 180), latitude-major.  ``grid_points(5)`` is
    the 36 x 72 global grid."""
    dlat = float(lat_step_deg)
    dlon = dlat if lon_step_deg is None else float(lon_step_deg)
    if not (np.isfinite(dlat) and np.isfinite(dlon) and dlat > 0.0 and 0.0 < dlon <= 360.0):
        raise ValueError("grid steps must be positive (the longitude step at most 360)")
    lo, hi = max(-90.0, float(lat_range[0])), min(90.0, float(lat_range[1]))
    if not lo < hi or not np.isfinite(float(alt_km)):
        raise ValueError("lat_range must be (south, north) with south < north, alt_km finite")
    edges = lo + dlat * np.arange(int(np.ceil((hi - lo) / dlat - 1e-9)) + 1)
    lat = 0.5 * (edges[:-1] + np.minimum(edges[1:], hi))
    lon = -180.0 + dlon * (np.arange(int(np.ceil(360.0 / dlon - 1e-9))) + 0.5)
    lon = lon[lon < 180.0]
    out = np.empty((len(lat), len(lon), 3))
    out[..., 0] = lat[:, None]
    out[..., 1] = lon[None, :]
    out[..., 2] = float(alt_km)
    return out.reshape(-1, 3)


# eclipses(): one row per shadow interval
ECLIPSE_DTYPE = np.dtype([("sat", "<u4"), ("entry", "<f8"), ("exit", "<f8"), ("flags", "<u4")])


def sun_position(jd):
    """The Sun's position at Julian date(s) ``jd`` (UTC), km, in the TEME frame of ``propagate(output="teme")``: shape
    ``jd.shape + (3,)``.  The low-precision series of the Astronomical Almanac (0.01 degrees, 1950-2050): the model
    :func:`eclipses` uses.  A host function; no GPU involved."""
    return _native.sun_position(jd)


def eclipses(source, times, *, kind="umbra", start_time=None, state=False, norad_id=None, fetch=None, allow_network=False):
    """Earth-shadow intervals of every satellite during ``times`` (minutes from ``start_time``, default now; strictly
    increasing).  ``kind``: ``"umbra"`` (full shadow) or ``"penumbra"`` (any shadow, the umbra included).

    Returns a numpy structured array, one row per interval, sorted by (sat, entry): ``sat`` (output row), ``entry``, ``exit``
    (minutes from ``start_time``, refined between grid points by cubic Hermite interpolation of the distance to the shadow
    cone and its rate) and ``flags`` (1: already in shadow at the first time, 2: still in shadow at the last, 4: cut by a
    failed propagation; an open end is the grid time).  With ``state=True`` also the ``(n_satellites, n_times)`` uint8 matrix
    of the grid points: 0 sunlit, 1 penumbra only, 2 umbra, 255 propagation failed.  Conical shadow of a spherical Earth; no
    oblateness, refraction or light time.  The propagation and the search run on the GPU; only the records come back."""
    if kind not in _native.SHADOW_KINDS:
        raise ValueError("kind must be 'umbra' or 'penumbra'")
    minutes = np.ascontiguousarray(times, dtype=np.float64)
    if minutes.ndim != 1 or (len(minutes) > 1 and not (np.diff(minutes) > 0).all()):
        raise ValueError("times must be strictly increasing")
    const = source if isinstance(source, Constellation) else Constellation(source, norad_id=norad_id, fetch=fetch,
                                                                           allow_network=allow_network)
    minutes, offsets, start = _minutes_and_offsets(const, minutes, start_time)
    find = lambda room: const._dev.find_eclipses(minutes, offsets, reference_jd=start, kind=_native.SHADOW_KINDS[kind],  # noqa: E731
                                                 max_eclipses=room, state=state)
    res = find(32)
    if res[1].size and int(res[1].max()) > res[0].shape[1]:  # more intervals than room: once more with room for all of them
        res = find(int(res[1].max()))
    rec, cnt = res[0], res[1]
    idx = np.repeat(np.arange(len(cnt), dtype=np.intp), cnt)
    k = np.concatenate([np.arange(c, dtype=np.intp) for c in cnt]) if len(cnt) else np.zeros(0, dtype=np.intp)
    r = rec[idx, k] if len(idx) else rec.reshape(-1)[:0]
    out = np.empty(len(idx), dtype=ECLIPSE_DTYPE)
    out["sat"], out["entry"], out["exit"], out["flags"] = idx, r["t_entry_min"], r["t_exit_min"], r["flags"]
    return (out, res[2]) if state else out


# access(): one row per line-of-sight window
ACCESS_DTYPE = np.dtype([("sat", "<u4"), ("start", "<f8"), ("end", "<f8"), ("min_range", "<f8"), ("t_min_range", "<f8"),
                         ("flags", "<u4")])


def access(source, times, target, *, grazing_altitude=0.0, max_range=None, start_time=None, state=False, norad_id=None, fetch=None,
           allow_network=False):
    """Line-of-sight access windows between satellite ``target`` (an output row, as for ``screen()``) and every other
    satellite during ``times`` (minutes from ``start_time``, default now; strictly increasing): the straight line between the
    two stays at least ``grazing_altitude`` km above a spherical Earth of 6378.137 km and, with ``max_range`` (km) set, is no
    longer than that.

    Returns a numpy structured array, one row per window, sorted by (sat, start): ``sat`` (output row), ``start``, ``end``
    (minutes from ``start_time``, refined between grid points by cubic Hermite interpolation of the clearance -- or the range
    margin -- and its rate), ``min_range`` (km, the smallest distance at a grid time inside the window) and ``t_min_range``
    (that grid time), and ``flags`` (1: already in access at the first time, 2: still in access at the last, 4: cut by a
    failed propagation of either satellite; an open end is the grid time).  The target's own row has no windows.  With
    ``state=True`` also the ``(n_satellites, n_times)`` uint8 matrix of the grid points: 0 Earth in the way, 1 clear line but
    beyond ``max_range``, 2 access, 255 propagation failed.  No oblateness, refraction or light time.  The propagation and the
    search run on the GPU; only the records come back."""
    try:
        row = int(target)
    except (TypeError, ValueError):
        raise ValueError("target must be the index of a satellite") from None
    if row < 0 or row != target:
        raise ValueError("target must be the index of a satellite")
    h = float(grazing_altitude)
    if not (np.isfinite(h) and h >= 0.0):
        raise ValueError("grazing_altitude must be finite and >= 0 km")
    if max_range is not None and not float(max_range) > 0.0:
        raise ValueError("max_range must be > 0 km, or None for no limit")
    minutes = np.ascontiguousarray(times, dtype=np.float64)
    if minutes.ndim != 1 or (len(minutes) > 1 and not (np.diff(minutes) > 0).all()):
        raise ValueError("times must be strictly increasing")
    const = source if isinstance(source, Constellation) else Constellation(source, norad_id=norad_id, fetch=fetch,
                                                                           allow_network=allow_network)
    if row >= const.num_satellites:
        raise ValueError("target index out of range")
    minutes, offsets, start = _minutes_and_offsets(const, minutes, start_time)
    find = lambda room: const._dev.find_access(minutes, row, offsets, grazing_alt_km=h, max_range_km=max_range,  # noqa: E731
                                               max_windows=room, state=state)
    res = find(32)
    if res[1].size and int(res[1].max()) > res[0].shape[1]:  # more windows than room: once more with room for all of them
        res = find(int(res[1].max()))
    rec, cnt = res[0], res[1]
    idx = np.repeat(np.arange(len(cnt), dtype=np.intp), cnt)
    k = np.concatenate([np.arange(c, dtype=np.intp) for c in cnt]) if len(cnt) else np.zeros(0, dtype=np.intp)
    r = rec[idx, k] if len(idx) else rec.reshape(-1)[:0]
    out = np.empty(len(idx), dtype=ACCESS_DTYPE)
    out["sat"], out["start"], out["end"], out["flags"] = idx, r["t_start_min"], r["t_end_min"], r["flags"]
    out["min_range"], out["t_min_range"] = r["min_range_km"], minutes[r["grid_min_range"]] if len(idx) else 0.0
    return (out, res[2]) if state else out


# conjunctions(): one row per refined close approach
CONJUNCTION_DTYPE = np.dtype([("target", "<u4"), ("sat", "<u4"), ("tca", "<f8"), ("miss", "<f8"), ("rel_speed", "<f8"),
                              ("grid_index", "<u4")])
_CONJUNCTION_ROOM = 4096  # records the first call of conjunctions() has room for


def conjunctions(source, times, targets, threshold=10.0, *, start_time=None, norad_id=None, fetch=None, allow_network=False):
    """Refined close approaches between the satellites ``targets`` (an output row or a sequence of them, as for ``screen()``;
    repeats allowed) and every other satellite during ``times`` (minutes from ``start_time``, default now; strictly
    increasing): every approach whose miss distance is below ``threshold`` km.

    Returns a numpy structured array, one row per approach, sorted by (target, sat, tca): ``target`` and ``sat`` (output
    rows), ``tca`` (minutes from ``start_time``), ``miss`` (km) and ``rel_speed`` (km/s) at the closest approach, and
    ``grid_index`` (the grid interval ``[grid_index, grid_index + 1]`` that holds it).  An approach is looked for in every grid
    interval at whose left end the two close in and at whose right end they no longer do; inside it the relative track is the
    cubic Hermite interpolant of the propagated states, so the answer sees between grid points (unlike ``screen()``, which
    reports distances AT grid times).  Not reported: a minimum at the first or last time, next to a failed propagation of
    either satellite, or in an interval that also holds a maximum.  No light time, covariance or collision probability.  The
    propagation and the search run on the GPU; only the records come back."""
    try:
        rows = np.atleast_1d(np.asarray(targets))
        ok = rows.ndim == 1 and rows.size > 0 and rows.dtype != np.bool_ and np.issubdtype(rows.dtype, np.integer) and not (rows < 0).any()
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("targets must be a satellite index or a non-empty sequence of them")
    thr = float(threshold)
    if not (np.isfinite(thr) and thr > 0.0):
        raise ValueError("threshold must be finite and > 0 km")
    minutes = np.ascontiguousarray(times, dtype=np.float64)
    if minutes.ndim != 1 or (len(minutes) > 1 and not (np.diff(minutes) > 0).all()):
        raise ValueError("times must be strictly increasing")
    const = source if isinstance(source, Constellation) else Constellation(source, norad_id=norad_id, fetch=fetch,
                                                                           allow_network=allow_network)
    if int(rows.max()) >= const.num_satellites:
        raise ValueError("target index out of range")
    minutes, offsets, start = _minutes_and_offsets(const, minutes, start_time)
    find = lambda room: const._dev.find_conjunctions(minutes, rows, thr, offsets, max_events=room)  # noqa: E731
    rec, n_ev = find(_CONJUNCTION_ROOM)
    if n_ev > len(rec):  # more events than room: once more with room for all of them
        rec, n_ev = find(n_ev)
    out = np.empty(len(rec), dtype=CONJUNCTION_DTYPE)
    out["target"], out["sat"], out["grid_index"] = rows[rec["target"]], rec["sat"], rec["grid_index"]
    out["tca"], out["miss"], out["rel_speed"] = rec["t_tca_min"], rec["miss_km"], rec["rel_speed_km_s"]
    return out[np.lexsort((out["tca"], out["sat"], out["target"]))]  # (slots of the same row interleave)


def screen(source, times, threshold=10.0, *, target=None, start_time=None, norad_id=None, fetch=None, allow_network=False):
    """Screen a constellation for conjunction events (reference __init__.py L535-658).

    ``target`` set: fused propagate+screen on the GPU against that satellite; returns
    ``(min_distances (n_sats,) float64 km, min_t_indices (n_sats,) uint32)`` -- a satellite that never
    comes within ``threshold`` (and the target itself) reports ``threshold`` and index 0.
    ``target`` None: all-vs-all; returns ``(pairs (k, 2) uint32, t_indices (k,) uint32)`` for every pair
    closer than ``threshold`` km at a grid time, sorted by (t, s, other).  Positions stay in HBM.
    Deep-space members take part in both modes (the reference's fused routine covers pure-SGP4
    constellations only and falls back to propagate-then-screen otherwise, L655-658)."""
    const = source if isinstance(source, Constellation) else Constellation(source, norad_id=norad_id, fetch=fetch,
                                                                           allow_network=allow_network)
    minutes, offsets, start = _minutes_and_offsets(const, times, start_time)
    if target is not None:
        return const._dev.screen_target(minutes, int(target), float(threshold), offsets, reference_jd=start)
    return const._dev.screen_all(minutes, float(threshold), offsets)


def coarse_screen(positions, num_sats, threshold, valid_mask=None):
    """``_astroz.coarse_screen(positions, num_sats, threshold, [valid_mask])`` (bindings/python/src/
    conjunction.zig L152-260): positions satellite-major ``(num_sats, n_times, 3)`` float64 (any shape
    with that memory order); returns ``(pairs, t_indices)`` as lists like the reference -- sorted by
    (t, s, other) rather than in hash-chain order."""
    pos = np.ascontiguousarray(positions, dtype=np.float64)
    if num_sats <= 0 or pos.size % (num_sats * 3) != 0:
        raise ValueError("positions array size not consistent with num_sats")
    pos = pos.reshape(num_sats, pos.size // (num_sats * 3), 3)
    pairs, tt = _native.coarse_screen(pos, threshold, valid_mask, layout=_native.SAT_MAJOR)
    return [tuple(int(x) for x in p) for p in pairs], [int(x) for x in tt]


# ---- the four closed-form orbital scalars of the reference's module surface (bindings/python/src/main.zig L24-32 over
# src/calculations.zig L83-125) that libastroz_hip.so carries for C clients (orbital_*): same names, arguments and error
# behaviour.  bi_elliptic_transfer, lambert and propagate_numerical are mission analysis, off the propagation path.
EARTH_MU = 398600.5          # km^3/s^2, WGS84 (src/constants.zig L41-52)
EARTH_R_EQ = 6378.137        # km
EARTH_J2 = 0.00108262998905
SUN_MU = 1.32712e11          # km^3/s^2 (src/constants.zig L94-97; module constants of the reference's extension, main.zig L73-74)
MOON_MU = 4.90280e3          # km^3/s^2 (src/constants.zig L167-170)


def hohmann_transfer(mu, r1, r2):
    """hohmann_transfer(mu, r1, r2) -> dict(sma, dv1, dv2, total_dv, transfer_time, transfer_time_days); ValueError for
    non-positive radii or radii closer than 1,000 km (orbital_mechanics.zig L9-19)."""
    import ctypes as C

    class _H(C.Structure):
        _fields_ = [(k, C.c_double) for k in ("sma", "dv1", "dv2", "total_dv", "transfer_time", "transfer_time_days")]
    h = _H()
    rc = _native.lib().orbital_hohmann(float(mu), float(r1), float(r2), C.byref(h))
    if rc != 0:
        raise ValueError("invalid transfer parameters (radii must be positive and differ by >1000 km)")
    return {k: getattr(h, k) for k, _ in _H._fields_}


def _scalar(v, what, bad):
    if v < 0:   # (the c_api's -1.0 for an invalid radius / semi-major axis)
        raise ValueError(bad)
    return v


def orbital_velocity(mu, radius, sma=None):
    """Vis-viva speed; circular if `sma` is omitted."""
    return _scalar(_native.lib().orbital_velocity(float(mu), float(radius), 0.0 if sma is None else float(sma)),
                   "orbital_velocity", "invalid radius / semi-major axis")


def orbital_period(mu, sma):
    """Period in seconds (Kepler's third law)."""
    return _scalar(_native.lib().orbital_period(float(mu), float(sma)), "orbital_period", "invalid semi-major axis")


def escape_velocity(mu, radius):
    return _scalar(_native.lib().orbital_escape_velocity(float(mu), float(radius)), "orbital_escape_velocity", "invalid radius")


__all__ = ["__version__", "Tle", "Sgp4Constellation", "Constellation", "propagate", "passes", "station_passes", "coverage", "grid_points", "COVERAGE_DTYPE", "eclipses",
           "sun_position", "ECLIPSE_DTYPE", "access", "ACCESS_DTYPE", "conjunctions", "CONJUNCTION_DTYPE", "screen",
           "coarse_screen", "set_fetcher", "celestrak_url", "WGS72", "WGS84", "hohmann_transfer", "orbital_velocity", "orbital_period",
           "escape_velocity", "EARTH_MU", "EARTH_R_EQ", "EARTH_J2", "SUN_MU", "MOON_MU"]
# (the reference's package also re-exports bi_elliptic_transfer, lambert and propagate_numerical -- its orbital-mechanics and
# numerical-integration modules, outside the SGP4/SDP4 constellation path this package replaces: DESIGN.md 9)
