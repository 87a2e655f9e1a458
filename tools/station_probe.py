#!/usr/bin/env python3
"""Passes over S ground stations on config 2 (13,478 satellites x 1,440 one-minute steps, tools/topo_probe.py's catalog),
for S = 1, 4, 16, 64, timed with hipEvents around the device calls (median of --reps after two warm-up calls):

  - azh_find_passes_stations_device (one ECEF propagation into the row-window scratch + k_passes_stations per group);
  - the same S stations as S azh_find_passes_device calls (azh_set_observer before each);
  - azh_find_passes_stations_host (wall clock of the whole call, records copied back).

  tools/station_probe.py [--reps 10]     prints one JSON line"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from astroz_amd import _native, synth

REPS = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 10
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
    return float(np.median(ms))


def stations(s):
    """s sites spread over the globe (a golden-angle spiral in latitude / longitude), 10 degree masks."""
    k = np.arange(s)
    lat = np.degrees(np.arcsin(np.clip(1.0 - 2.0 * (k + 0.5) / s, -1.0, 1.0))) * (80.0 / 90.0)
    lon = (k * 137.50776405) % 360.0 - 180.0
    return np.stack([lat, lon, np.full(s, 0.2)], axis=1), np.full(s, 10.0)


def main():
    pairs = synth.synth_catalog(13478, 0)
    dev = _native.DeviceConstellation.from_tle_lines(pairs, _native.WGS72, 0)
    n = dev.n
    times = np.arange(1440.0)
    ref = synth.START_JD
    off = (ref - dev.epochs) * 1440.0
    stream = torch.cuda.Stream()  # (a stream of its own: the events below and the library's launches share it)
    torch.cuda.set_stream(stream)
    st = stream.cuda_stream
    out = {"config": "13478 x 1440, 1-min grid", "max_passes": MP, "runs": {}}
    d_out = torch.empty((64 * n * MP * 64,), dtype=torch.uint8, device="cuda")
    d_n = torch.empty((64 * n,), dtype=torch.int32, device="cuda")
    d_out1 = torch.empty((n * MP * 64,), dtype=torch.uint8, device="cuda")
    d_n1 = torch.empty((n,), dtype=torch.int32, device="cuda")
    for s in (1, 4, 16, 64):
        lla, mk = stations(s)
        r = {}
        r["stations_device_ms"] = timed(lambda: dev.find_passes_stations_device(times, off, lla, mk, d_out.data_ptr(), MP,
                                                                               d_n.data_ptr(), reference_jd=ref, stream=st))

        def singles():
            for k in range(s):
                dev.set_observer(*lla[k])
                dev.find_passes_device(times, off, d_out1.data_ptr(), MP, d_n1.data_ptr(), reference_jd=ref,
                                       min_elevation_deg=float(mk[k]), stream=st)
        r["singles_device_ms"] = timed(singles)
        ws = []
        for _ in range(REPS + 2):
            t0 = time.perf_counter()
            rec, cnt = dev.find_passes_stations(times, off, lla, mk, reference_jd=ref, max_passes=MP)
            ws.append((time.perf_counter() - t0) * 1e3)
        r["stations_host_ms"] = float(np.median(ws[2:]))
        r["passes"] = int(cnt.sum())
        r["max_passes_per_sat"] = int(cnt.max())
        out["runs"][str(s)] = r
    print(json.dumps(out))


if __name__ == "__main__":
    main()
