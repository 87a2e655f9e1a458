#!/usr/bin/env python3
"""Earth-shadow intervals on config 2 (13,478 satellites x 1,440 one-minute steps, tools/topo_probe.py's catalog), timed with
hipEvents around the device calls (median of --reps after two warm-up calls), all in one session:

  - azh_find_eclipses_device, umbra and any shadow, with and without the state matrix (one TEME propagation with velocities
    into the row-window scratch, the Sun table, k_eclipses per window);
  - azh_find_passes_device of the same build (topocentric propagation + k_passes), the yardstick;
  - the plain TEME satellite-major position + velocity propagation both contain (azh_propagate_device);
  - azh_find_eclipses_host (wall clock of the whole call, records and state copied back).

  tools/eclipse_probe.py [--reps 10] [--once]    prints one JSON line; --once makes five umbra calls with state and exits (the
                                                 run to put under rocprofv3 --kernel-trace --stats)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from astroz_amd import _native, synth

REPS = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 10
ME = 20


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
    d_out = torch.empty((n * ME * 32,), dtype=torch.uint8, device="cuda")
    d_n = torch.empty((n,), dtype=torch.int32, device="cuda")
    d_state = torch.empty((n, len(times)), dtype=torch.uint8, device="cuda")

    def ecl(kind, state):
        return lambda: dev.find_eclipses_device(times, off, d_out.data_ptr(), ME, d_n.data_ptr(), reference_jd=ref, kind=kind,
                                                d_state=d_state.data_ptr() if state else None, stream=st)
    if "--once" in sys.argv:
        for _ in range(5):
            ecl(0, True)()
        torch.cuda.synchronize()
        print(json.dumps({"calls": 5, "intervals": int(d_n.sum().item())}))
        return
    out = {"config": "13478 x 1440, 1-min grid", "max_eclipses": ME}
    for kind, name in ((0, "umbra"), (1, "penumbra")):
        out["eclipses_%s_device_ms" % name] = timed(ecl(kind, False))
        out["eclipses_%s_state_device_ms" % name] = timed(ecl(kind, True))
        cnt = d_n.cpu().numpy()
        out["%s_intervals" % name] = int(cnt.sum())
        out["%s_max_per_sat" % name] = int(cnt.max())
    d_pass = torch.empty((n * 16 * 64,), dtype=torch.uint8, device="cuda")
    dev.set_observer(47.3, 8.5, 0.4)
    out["passes_device_ms"] = timed(lambda: dev.find_passes_device(times, off, d_pass.data_ptr(), 16, d_n.data_ptr(), reference_jd=ref,
                                                                   min_elevation_deg=10.0, stream=st))
    out["passes"] = int(d_n.sum().item())
    d_pos = torch.empty((n, len(times), 3), dtype=torch.float64, device="cuda")
    d_vel = torch.empty_like(d_pos)
    d_err = torch.empty((n, len(times)), dtype=torch.uint8, device="cuda")
    out["propagate_teme_sat_major_ms"] = timed(lambda: dev.propagate_device(
        times, off, d_pos.data_ptr(), d_vel.data_ptr(), mode=_native.OUT_TEME, reference_jd=ref, layout=_native.SAT_MAJOR,
        d_err=d_err.data_ptr(), stream=st))
    ws = []
    for _ in range(REPS + 2):
        t0 = time.perf_counter()
        rec, cnt, state = dev.find_eclipses(times, off, reference_jd=ref, kind=0, max_eclipses=ME, state=True)
        ws.append((time.perf_counter() - t0) * 1e3)
    out["eclipses_umbra_state_host_ms"] = float(np.median(ws[2:]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
