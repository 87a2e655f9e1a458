#!/usr/bin/env python3
"""Ground coverage on config 2 (13,478 satellites x 1,440 one-minute steps, tools/topo_probe.py's catalog) over --points
ground points (default 1,000: tools/station_probe.py's spiral, 10 degree masks):

  (a) azh_coverage_device, statistics only -- hipEvents around the call, median of --reps after two warm-up calls;
  (b) the route to the same counts without it: azh_find_passes_stations_host with max_passes = 16, as many stations per call
      as astroz_amd.station_passes takes (256 MiB of records), and the records rasterised on the host -- wall clock of the
      whole route, median of --reps-b after one warm-up pass (it takes seconds per pass), and its counts compared with (a)'s;
  (c) the propagation alone: azh_propagate_device, AZ_OUT_ECEF positions and error codes, satellite-major -- what
      pass_windows launches for (a); hipEvents, median of --reps.

  tools/coverage_probe.py [--points 1000] [--reps 10] [--reps-b 10] [--skip-b]     prints one JSON line"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import astroz_amd
from astroz_amd import _native, synth


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


POINTS, REPS, REPS_B = arg("--points", 1000), arg("--reps", 10), arg("--reps-b", 10)
MP = 16


def timed(fn, reps=REPS):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), [round(x, 3) for x in ms]


def spiral(s):
    """s sites spread over the globe (a golden-angle spiral in latitude / longitude), 10 degree masks."""
    k = np.arange(s)
    lat = np.degrees(np.arcsin(np.clip(1.0 - 2.0 * (k + 0.5) / s, -1.0, 1.0))) * (80.0 / 90.0)
    lon = (k * 137.50776405) % 360.0 - 180.0
    return np.stack([lat, lon, np.full(s, 0.2)], axis=1), np.full(s, 10.0)


def rasterise(rec, cnt, n_times):
    out = np.zeros((rec.shape[0], n_times + 1), dtype=np.int64)
    for st in range(rec.shape[0]):
        r = rec[st][np.arange(rec.shape[2]) < np.minimum(cnt[st], rec.shape[2])[:, None]]
        np.add.at(out[st], r["grid_rise"], 1)
        np.add.at(out[st], r["grid_set"].astype(np.int64) + 1, -1)
    return np.cumsum(out, axis=1)[:, :n_times].astype(np.uint32)


def main():
    pairs = synth.synth_catalog(13478, 0)
    dev = _native.DeviceConstellation.from_tle_lines(pairs, _native.WGS72, 0)
    n = dev.n
    times = np.arange(1440.0)
    ref = synth.START_JD
    off = (ref - dev.epochs) * 1440.0
    pts, mk = spiral(POINTS)
    stream = torch.cuda.Stream()  # (a stream of its own: the events below and the library's launches share it)
    torch.cuda.set_stream(stream)
    st = stream.cuda_stream
    out = {"config": "13478 x 1440, 1-min grid", "points": POINTS, "pair_tests": n * len(times) * POINTS}

    d_stats = torch.empty((POINTS * _native.COVERAGE_DTYPE.itemsize,), dtype=torch.uint8, device="cuda")
    d_counts = torch.empty((POINTS * len(times),), dtype=torch.int32, device="cuda")
    a_ms, a_all = timed(lambda: dev.coverage_device(times, off, pts, mk, d_stats.data_ptr(), None, reference_jd=ref, stream=st))
    out["coverage_stats_only_ms"], out["coverage_stats_only_all_ms"] = a_ms, a_all
    dev.coverage_device(times, off, pts, mk, d_stats.data_ptr(), d_counts.data_ptr(), reference_jd=ref, stream=st)
    stream.synchronize()
    counts = d_counts.cpu().numpy().view(np.uint32).reshape(POINTS, len(times))
    out["in_view_total"] = int(counts.sum())

    d_pos = torch.empty((n * len(times) * 3,), dtype=torch.float64, device="cuda")
    d_err = torch.empty((n * len(times),), dtype=torch.uint8, device="cuda")
    c_ms, c_all = timed(lambda: dev.propagate_device(times, off, d_pos.data_ptr(), None, mode=_native.OUT_ECEF, reference_jd=ref,
                                                     layout=_native.SAT_MAJOR, d_err=d_err.data_ptr(), stream=st))
    out["propagation_only_ms"], out["propagation_only_all_ms"] = c_ms, c_all
    out["count_and_stats_ms"] = a_ms - c_ms
    out["pair_tests_per_s_whole_call"] = out["pair_tests"] / (a_ms * 1e-3)
    out["pair_tests_per_s_kernels"] = out["pair_tests"] / max(1e-9, (a_ms - c_ms) * 1e-3)
    del d_pos, d_err

    if "--skip-b" not in sys.argv:
        per_call = max(1, astroz_amd._STATION_CALL_BYTES // (n * MP * _native.PASS_DTYPE.itemsize))
        ws, same = [], True
        for rep in range(REPS_B + 1):  # (the first one warms up)
            t0 = time.perf_counter()
            got = np.empty_like(counts)
            for lo in range(0, POINTS, per_call):
                rec, cnt = dev.find_passes_stations(times, off, pts[lo:lo + per_call], mk[lo:lo + per_call], reference_jd=ref,
                                                    max_passes=MP)
                got[lo:lo + per_call] = rasterise(rec, cnt, len(times))
                same = same and int(cnt.max()) <= MP  # (room for every pass)
            ws.append((time.perf_counter() - t0) * 1e3)
            same = same and bool(np.array_equal(got, counts))
        out["stations_route_ms"] = float(np.median(ws[1:]))
        out["stations_route_all_ms"] = [round(x, 1) for x in ws[1:]]
        out["stations_route_calls"] = (POINTS + per_call - 1) // per_call
        out["stations_route_same_counts"] = same
    print(json.dumps(out))


if __name__ == "__main__":
    main()
