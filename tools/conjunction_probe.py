#!/usr/bin/env python3
"""Refined close approaches on config 2 (13,478 satellites x 1,440 one-minute steps, tools/topo_probe.py's catalog), 10 km,
K = 1 / 16 / 64 targets spread over the catalog, timed with hipEvents around the device calls (median of --reps after two
warm-up calls), all in one session:

  - azh_find_conjunctions_device (one TEME propagation with velocities into the row-window scratch, the targets' one-row
    launches, k_conjunctions per window);
  - K calls of azh_screen_target_device of the same build: a cost yardstick only -- they answer a weaker question (the smallest
    distance AT a grid time);
  - the plain TEME satellite-major position + velocity propagation the finder contains (azh_propagate_device).

  tools/conjunction_probe.py [--reps 20] [--once K]    prints one JSON line; --once K makes five K-target calls and exits (the
                                                       run to put under rocprofv3 --kernel-trace --stats)"""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from astroz_amd import _native, synth

REPS = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 20
ROOM = 1 << 16
THRESHOLD_KM = 10.0


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
    d_out = torch.empty((ROOM * 40,), dtype=torch.uint8, device="cuda")
    d_n = torch.zeros((1,), dtype=torch.int32, device="cuda")
    d_dist = torch.empty((n,), dtype=torch.float64, device="cuda")
    d_ti = torch.empty((n,), dtype=torch.int32, device="cuda")
    L = _native.lib()

    def targets(K):
        return np.linspace(0, n - 1, K).astype(np.int64) if K > 1 else np.array([0])

    def conj(K):
        tg = targets(K)
        return lambda: dev.find_conjunctions_device(times, tg, THRESHOLD_KM, off, d_out.data_ptr(), ROOM, d_n.data_ptr(), stream=st)

    def screens(K):
        tg = targets(K)

        def run():
            for t in tg:
                _native.check(L.azh_screen_target_device(dev._h, times.ctypes.data, len(times), off.ctypes.data, int(t), THRESHOLD_KM,
                                                         ref, d_dist.data_ptr(), d_ti.data_ptr(), C.c_void_p(st)),
                              "azh_screen_target_device")
        return run
    if "--once" in sys.argv:
        K = int(sys.argv[sys.argv.index("--once") + 1])
        for _ in range(5):
            conj(K)()
        torch.cuda.synchronize()
        print(json.dumps({"calls": 5, "targets": K, "events": int(d_n.item())}))
        return
    out = {"config": "13478 x 1440, 1-min grid", "threshold_km": THRESHOLD_KM, "reps": REPS}
    for K in (1, 16, 64):
        out["conjunctions_K%d_device_ms" % K] = timed(conj(K))
        out["K%d_events" % K] = int(d_n.item())
        out["screen_target_x%d_device_ms" % K] = timed(screens(K))
        out["K%d_grid_points_below_threshold" % K] = int((d_dist < THRESHOLD_KM).sum().item())  # (of the last target only)
    d_pos = torch.empty((n, len(times), 3), dtype=torch.float64, device="cuda")
    d_vel = torch.empty_like(d_pos)
    d_err = torch.empty((n, len(times)), dtype=torch.uint8, device="cuda")
    out["propagate_teme_sat_major_ms"] = timed(lambda: dev.propagate_device(
        times, off, d_pos.data_ptr(), d_vel.data_ptr(), mode=_native.OUT_TEME, reference_jd=ref, layout=_native.SAT_MAJOR,
        d_err=d_err.data_ptr(), stream=st))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
