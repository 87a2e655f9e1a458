#!/usr/bin/env python3
"""Line-of-sight access windows on config 2 (13,478 satellites x 1,440 one-minute steps, tools/topo_probe.py's catalog), timed
with hipEvents around the device calls (median of --reps after two warm-up calls), all in one session:

  - azh_find_access_device, target = catalog row 0, 100 km grazing altitude, no range limit and 5,000 km, with and without
    the state matrix (one TEME propagation with velocities into the row-window scratch, the target's one-row launch, k_access
    per window);
  - azh_find_eclipses_device of the same build (the same propagation + the Sun table + k_eclipses), the yardstick;
  - the plain TEME satellite-major position + velocity propagation both contain (azh_propagate_device);
  - azh_find_access_host (wall clock of the whole call, records and state copied back).

  tools/access_probe.py [--reps 20] [--once]    prints one JSON line; --once makes five 5,000-km calls with state and exits (the
                                                run to put under rocprofv3 --kernel-trace --stats)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from astroz_amd import _native, synth

REPS = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 20
ROOM = 32
TARGET, GRAZE_KM = 0, 100.0


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
    stream = torch.cuda.Stream()  # (a stream of its own: the events below and the library's launches share it)
    torch.cuda.set_stream(stream)
    st = stream.cuda_stream
    d_out = torch.empty((n * ROOM * 40,), dtype=torch.uint8, device="cuda")
    d_n = torch.empty((n,), dtype=torch.int32, device="cuda")
    d_state = torch.empty((n, len(times)), dtype=torch.uint8, device="cuda")

    def acc(max_range, state):
        return lambda: dev.find_access_device(times, TARGET, off, d_out.data_ptr(), ROOM, d_n.data_ptr(), grazing_alt_km=GRAZE_KM,
                                              max_range_km=max_range, d_state=d_state.data_ptr() if state else None, stream=st)
    if "--once" in sys.argv:
        for _ in range(5):
            acc(5000.0, True)()
        torch.cuda.synchronize()
        print(json.dumps({"calls": 5, "windows": int(d_n.sum().item())}))
        return
    out = {"config": "13478 x 1440, 1-min grid", "target": TARGET, "grazing_alt_km": GRAZE_KM, "max_windows": ROOM, "reps": REPS}
    for max_range, name in ((None, "unlimited"), (5000.0, "5000km")):
        out["access_%s_device_ms" % name] = timed(acc(max_range, False))
        out["access_%s_state_device_ms" % name] = timed(acc(max_range, True))
        cnt = d_n.cpu().numpy()
        out["%s_windows" % name] = int(cnt.sum())
        out["%s_max_per_sat" % name] = int(cnt.max())
    d_ecl = torch.empty((n * 20 * 32,), dtype=torch.uint8, device="cuda")
    out["eclipses_umbra_device_ms"] = timed(lambda: dev.find_eclipses_device(times, off, d_ecl.data_ptr(), 20, d_n.data_ptr(),
                                                                              reference_jd=ref, kind=0, stream=st))
    out["eclipses_umbra_state_device_ms"] = timed(lambda: dev.find_eclipses_device(times, off, d_ecl.data_ptr(), 20, d_n.data_ptr(),
                                                                                    reference_jd=ref, kind=0, d_state=d_state.data_ptr(),
                                                                                    stream=st))
    d_pos = torch.empty((n, len(times), 3), dtype=torch.float64, device="cuda")
    d_vel = torch.empty_like(d_pos)
    d_err = torch.empty((n, len(times)), dtype=torch.uint8, device="cuda")
    out["propagate_teme_sat_major_ms"] = timed(lambda: dev.propagate_device(
        times, off, d_pos.data_ptr(), d_vel.data_ptr(), mode=_native.OUT_TEME, reference_jd=ref, layout=_native.SAT_MAJOR,
        d_err=d_err.data_ptr(), stream=st))
    ws = []
    for _ in range(REPS + 2):
        t0 = time.perf_counter()
        dev.find_access(times, TARGET, off, grazing_alt_km=GRAZE_KM, max_range_km=5000.0, max_windows=ROOM, state=True)
        ws.append((time.perf_counter() - t0) * 1e3)
    out["access_5000km_state_host_ms"] = float(np.median(ws[2:]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
