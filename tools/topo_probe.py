#!/usr/bin/env python3
"""Topocentric output and the pass finder on config 2 (13,478 satellites x 1,440 one-minute steps), timed with hipEvents
around the device calls (median of --reps after two warm-up calls):

  - AZ_OUT_TOPOCENTRIC satellite-major and time-major, with and without rates (azh_propagate_device_cached; ECEF beside it
    for comparison);
  - azh_find_passes_device (the topocentric propagation into the row-window scratch + k_passes, records in HBM);
  - azh_find_passes_host (wall clock of the whole call, records copied back).

  tools/topo_probe.py [--reps 20]     prints one JSON line"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from astroz_amd import _native, synth

REPS = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 20
OBS = (47.3, 8.5, 0.4)


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


def main():
    pairs = synth.synth_catalog(13478, 0)
    dev = _native.DeviceConstellation.from_tle_lines(pairs, _native.WGS72, 0)
    n = dev.n
    times = np.arange(1440.0)
    ref = synth.START_JD
    off = (ref - dev.epochs) * 1440.0
    dev.set_observer(*OBS)
    p = torch.empty((n * len(times) * 3,), dtype=torch.float64, device="cuda")
    v = torch.empty_like(p)
    stream = torch.cuda.Stream()  # (a stream of its own: the events below and the library's launches share it)
    torch.cuda.set_stream(stream)
    st = stream.cuda_stream
    out = {"config": "13478 x 1440, 1-min grid", "observer": OBS}
    for name, mode in (("ecef", _native.OUT_ECEF), ("topocentric", _native.OUT_TOPOCENTRIC)):
        for lay_name, lay in (("sat_major", _native.SAT_MAJOR), ("time_major", _native.TIME_MAJOR)):
            for vel in (False, True):
                dv = v.data_ptr() if vel else None
                dev.propagate_device(times, off, p.data_ptr(), dv, mode=mode, reference_jd=ref, layout=lay, stream=st)
                out["%s_%s_%s_ms" % (name, lay_name, "pos_vel" if vel else "pos")] = timed(
                    lambda: dev.propagate_device_cached(p.data_ptr(), dv, layout=lay, stream=st))
    mp = 16
    d_out = torch.empty((n * mp * 64,), dtype=torch.uint8, device="cuda")
    d_n = torch.empty((n,), dtype=torch.int32, device="cuda")
    out["find_passes_device_ms"] = timed(lambda: dev.find_passes_device(times, off, d_out.data_ptr(), mp, d_n.data_ptr(),
                                                                        reference_jd=ref, min_elevation_deg=10.0, stream=st))
    ws = []
    for k in range(REPS + 2):
        t0 = time.perf_counter()
        rec, cnt = dev.find_passes(times, off, reference_jd=ref, min_elevation_deg=10.0, max_passes=mp)
        ws.append((time.perf_counter() - t0) * 1e3)
    out["find_passes_host_ms"] = float(np.median(ws[2:]))
    out["passes"] = int(cnt.sum())
    out["max_passes_per_sat"] = int(cnt.max())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
