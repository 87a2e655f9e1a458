#!/usr/bin/env python3
"""CPU study of k_rows_fast's two loop bodies on a whole catalog (tests/host_emul/emul_tiers.cpp: the device headers
compiled for the host): the tier histogram of the window plan, the worst difference from the oracle per body, and the
largest difference between the eps body and the general body on the same windows.
usage: tools/tier_study.py [n_sats] [n_times] [tile_c] [tile_e] [seed]"""
import ctypes as C, os, subprocess, sys, tempfile
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from astroz_amd import synth
from oracle import oracle

n_sats = int(sys.argv[1]) if len(sys.argv) > 1 else 13478
n_times = int(sys.argv[2]) if len(sys.argv) > 2 else 1440
tile_c = int(sys.argv[3]) if len(sys.argv) > 3 else 768
tile_e = int(sys.argv[4]) if len(sys.argv) > 4 else 256
seed = int(sys.argv[5]) if len(sys.argv) > 5 else 20260926
src = os.path.join(ROOT, "tests", "host_emul", "emul_tiers.cpp")
lib = os.path.join(tempfile.mkdtemp(), "libemul_tiers.so")
subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wno-unknown-pragmas", "-o", lib, src])
E = C.CDLL(lib)
E.emul_tiers_init.restype = C.c_uint
E.emul_tiers_init.argtypes = [C.c_void_p] * 3
E.emul_tiers_row.restype = None
E.emul_tiers_row.argtypes = [C.c_void_p, C.c_uint, C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int,
                             C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
g = np.array([6378.135, 0.001082616, -0.00000165597, 0.0743669161331734132, -0.00234506972242078, 0.0743669161331734132 * 6378.135 / 60.0])
pairs = synth.synth_catalog(n_near=n_sats, n_deep=0, seed=seed)
tles = [oracle.parse_lines(a, b) for a, b in pairs]
cat = oracle.Catalog(tles, 1)
off = (synth.START_JD - cat.epoch_jd) * 1440.0
times = np.arange(n_times, dtype=np.float64)
_, p0, v0 = cat.propagate(times, off, layout=oracle.SAT_MAJOR, threads=os.cpu_count())
nf = E.emul_tiers_num_fields()
names = ("general", "eps", "eccentric")
windows = dict.fromkeys(names + ("rejected",), 0)
worst = {k: [0.0, 0.0] for k in names}
cross = [0.0, 0.0]
out = np.zeros((n_times, 6)); outg = np.zeros((n_times, 6)); tier = np.zeros(n_times, dtype=np.int32); tg = np.zeros(n_times, dtype=np.int32)
probe = np.zeros((n_times, 4))
for i, t in enumerate(tles):
    raw = np.array([t.epoch_jd, t.mm_revday, t.ecc, t.incl_deg, t.raan_deg, t.argp_deg, t.ma_deg, t.bstar])
    fields = np.zeros(nf)
    flags = E.emul_tiers_init(raw.ctypes.data, g.ctypes.data, fields.ctypes.data)
    ecc = 1 if ((flags >> 12) & 3) else 0
    tile = tile_e if ecc else tile_c
    E.emul_tiers_row(fields.ctypes.data, flags, g.ctypes.data, times[0] + off[i], 1.0, n_times, tile, ecc, -1, None, 0.0,
                     out.ctypes.data, tier.ctypes.data, probe.ctypes.data)
    for w in range(0, n_times, tile):
        v = int(tier[w])
        windows["rejected" if v < 0 else ("eccentric" if ecc else names[v])] += 1
    for v in (0, 1):
        sel = tier == v
        if sel.any():
            k = "eccentric" if ecc else names[v]
            worst[k][0] = max(worst[k][0], np.abs(out[sel, :3] - p0[i][sel]).max())
            worst[k][1] = max(worst[k][1], np.abs(out[sel, 3:] - v0[i][sel]).max())
    cheap = tier >= 1
    if cheap.any():
        E.emul_tiers_row(fields.ctypes.data, flags, g.ctypes.data, times[0] + off[i], 1.0, n_times, tile, ecc, 0, None, 0.0,
                         outg.ctypes.data, tg.ctypes.data, probe.ctypes.data)
        cross[0] = max(cross[0], np.abs(outg[cheap, :3] - out[cheap, :3]).max())
        cross[1] = max(cross[1], np.abs(outg[cheap, 3:] - out[cheap, 3:]).max())
tot = sum(windows.values())
print("%d satellites x %d one-minute steps, segments %d (near-circular) / %d (eccentric): %d windows" % (len(tles), n_times, tile_c, tile_e, tot))
for k in names + ("rejected",):
    line = "  %-9s %7d windows  %6.2f %%" % (k, windows[k], 100.0 * windows[k] / tot)
    if k in worst:
        line += "   max|dr| = %.3e km  max|dv| = %.3e km/s vs the oracle" % tuple(worst[k])
    print(line)
print("general body vs eps body on the eps windows: max|dr| = %.3e km, max|dv| = %.3e km/s" % tuple(cross))
