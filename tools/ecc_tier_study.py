#!/usr/bin/env python3
"""CPU study of the loop bodies of k_rows_fast's eccentric form on a whole catalog (tests/host_emul/emul_ecc_tiers.cpp: the
device headers compiled for the host): the histogram of eccentric windows per body (E1, E2, general, rejected), the worst
difference from the oracle per body over every eccentric row and every step, the same for the general body run on the same
windows (what every window ran before the tiers), and the largest difference between the two.
usage: tools/ecc_tier_study.py [n_sats] [n_times] [tile_e] [seed]
Importable: tests/test_ecc_tiers_cpu.py drives load() and run()."""
import ctypes as C, os, subprocess, sys, tempfile
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GRAV = np.array([6378.135, 0.001082616, -0.00000165597, 0.0743669161331734132, -0.00234506972242078, 0.0743669161331734132 * 6378.135 / 60.0])
BODIES = ("general", "E1", "E2")  # index = the tier value of fast_step.h (AZ_TIER_GENERAL, AZ_ETIER_E1, AZ_ETIER_E2)
PROBES = ("th", "em", "eps", "a_nd", "el2", "d0", "d1", "d2")
DELTA_MAX = 4.0e-6  # AZ_DELTA_MAX


def load(out_dir=None):
    """Compile the emulation and return its ctypes handle."""
    src = os.path.join(ROOT, "tests", "host_emul", "emul_ecc_tiers.cpp")
    lib = os.path.join(out_dir or tempfile.mkdtemp(), "libemul_ecc_tiers.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wno-unknown-pragmas", "-o", lib, src])
    E = C.CDLL(lib)
    E.emul_ecc_init.restype = C.c_uint
    E.emul_ecc_init.argtypes = [C.c_void_p] * 3
    E.emul_ecc_row.restype = None
    E.emul_ecc_row.argtypes = [C.c_void_p, C.c_uint, C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_double,
                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    E.emul_ecc_plan_tier.restype = C.c_int
    E.emul_ecc_plan_tier.argtypes = [C.c_void_p, C.c_uint, C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_double]
    assert E.emul_ecc_num_probes() == len(PROBES)
    return E


def plan_counts(E, oracle, pairs, t0, step, n, off, tile_c, tile_e, dmax=0.0):
    """The window plan of a whole catalog (near-earth rows that initialise) on the grid t0 + i step (+ off per satellite),
    counted as the library's two read-backs count it: ({"general", "eps", "ecc", "rejected"}, {"e1", "e2", "general"})."""
    nf = E.emul_ecc_num_fields()
    four = dict.fromkeys(("general", "eps", "ecc", "rejected"), 0)
    three = dict.fromkeys(("e1", "e2", "general"), 0)
    for i, (a, b) in enumerate(pairs):
        t = oracle.parse_lines(a, b)
        raw = np.array([t.epoch_jd, t.mm_revday, t.ecc, t.incl_deg, t.raan_deg, t.argp_deg, t.ma_deg, t.bstar])
        fields = np.zeros(nf)
        flags = E.emul_ecc_init(raw.ctypes.data, GRAV.ctypes.data, fields.ctypes.data)
        assert (flags & 0x1ff) == 0
        ecc = 1 if ((flags >> 12) & 3) else 0
        tile = tile_e if ecc else tile_c
        for t_lo in range(0, n, tile):
            v = E.emul_ecc_plan_tier(fields.ctypes.data, flags, GRAV.ctypes.data, t0 + off[i], step, t_lo, min(t_lo + tile, n), ecc, dmax)
            if v < 0:
                four["rejected"] += 1
            elif ecc:
                four["ecc"] += 1
                three[("general", "e1", "e2")[v]] += 1
            else:
                four[("general", "eps")[v]] += 1
    return four, three


def run(E, oracle, pairs, times, off_of_epochs, tile, quasi=False, threads=1):
    """The eccentric rows (class > 0) of `pairs` on the grid `times` (+ off_of_epochs(epoch_jd) per satellite), segments of
    `tile` points.  Returns a dict: idx (catalog rows taken), p0 / v0 (the oracle), tier [rows, n] (-1: rejected window), and
    per key "own" / "general" a tuple (out [rows, n, 6], bad [rows, n], probe [rows, n, 8])."""
    n = len(times)
    nf = E.emul_ecc_num_fields()
    tles = [oracle.parse_lines(a, b) for a, b in pairs]
    rows = []
    for i, t in enumerate(tles):
        raw = np.array([t.epoch_jd, t.mm_revday, t.ecc, t.incl_deg, t.raan_deg, t.argp_deg, t.ma_deg, t.bstar])
        fields = np.zeros(nf)
        flags = E.emul_ecc_init(raw.ctypes.data, GRAV.ctypes.data, fields.ctypes.data)
        if (flags & 0x1ff) == 0 and ((flags >> 12) & 3):
            rows.append((i, fields, flags))
    cat = oracle.Catalog([tles[i] for i, _, _ in rows], 1)
    off = off_of_epochs(cat.epoch_jd)
    step = (times[-1] - times[0]) / (n - 1)
    delta = (times - (times[0] + np.arange(n) * step)).astype(np.float32)
    assert np.abs(delta).max() <= DELTA_MAX and (quasi or not delta.any())
    _, p0, v0 = cat.propagate(times, off, layout=oracle.SAT_MAJOR, threads=threads)
    res = {"idx": np.array([i for i, _, _ in rows]), "p0": p0, "v0": v0, "tier": np.zeros((len(rows), n), dtype=np.int32)}
    for key, force in (("own", 0), ("general", 1)):
        o = np.full((len(rows), n, 6), np.nan)
        bad = np.zeros((len(rows), n), dtype=np.uint8)
        probe = np.zeros((len(rows), n, len(PROBES)))
        tier = np.zeros((len(rows), n), dtype=np.int32)
        for r, (_, fields, flags) in enumerate(rows):
            E.emul_ecc_row(fields.ctypes.data, flags, GRAV.ctypes.data, times[0] + off[r], step, n, tile, force,
                           delta.ctypes.data if quasi else None, DELTA_MAX if quasi else 0.0, o[r].ctypes.data, tier[r].ctypes.data,
                           bad[r].ctypes.data, probe[r].ctypes.data)
        if key == "own":
            res["tier"] = tier
        else:
            assert np.array_equal(tier, res["tier"])
        res[key] = (o, bad, probe)
    return res


def summarize(res, tile):
    """Per body: windows, points, worst |dr| / |dv| against the oracle of the body itself and of the general body on the same
    windows, and between the two.  Points the general body's predicate hands to the generic step are left out of ITS figures
    (the kernel never stores them)."""
    tier = res["tier"]
    o, bad, _ = res["own"]
    og, badg, _ = res["general"]
    out = {"rejected": {"windows": int((tier[:, ::tile] < 0).sum())}}
    for v, name in enumerate(BODIES):
        sel = tier == v
        d = {"windows": int((tier[:, ::tile] == v).sum()), "points": int(sel.sum())}
        if sel.any():
            keep = sel & (bad == 0)
            keepg = sel & (badg == 0)
            d["own"] = (float(np.abs(o[keep][:, :3] - res["p0"][keep]).max()), float(np.abs(o[keep][:, 3:] - res["v0"][keep]).max()))
            d["general"] = (float(np.abs(og[keepg][:, :3] - res["p0"][keepg]).max()), float(np.abs(og[keepg][:, 3:] - res["v0"][keepg]).max()))
            both = keep & keepg
            d["cross"] = (float(np.abs(og[both][:, :3] - o[both][:, :3]).max()), float(np.abs(og[both][:, 3:] - o[both][:, 3:]).max()))
            d["handed_over"] = int((sel & (bad != 0)).sum())
        out[name] = d
    acc = tier >= 0
    keep, keepg = acc & (bad == 0), acc & (badg == 0)
    out["all"] = {"own": (float(np.abs(o[keep][:, :3] - res["p0"][keep]).max()), float(np.abs(o[keep][:, 3:] - res["v0"][keep]).max())),
                  "general": (float(np.abs(og[keepg][:, :3] - res["p0"][keepg]).max()), float(np.abs(og[keepg][:, 3:] - res["v0"][keepg]).max()))}
    return out


def report(s, head):
    print(head)
    tot = sum(s[k]["windows"] for k in BODIES + ("rejected",))
    for name in ("E1", "E2", "general"):
        d = s[name]
        line = "  %-8s %6d windows %6.2f %%" % (name, d["windows"], 100.0 * d["windows"] / max(tot, 1))
        if "own" in d:
            line += "  vs oracle: this body %.3e km %.3e km/s | general body %.3e km %.3e km/s | between them %.3e km %.3e km/s" % (
                d["own"] + d["general"] + d["cross"])
            if d["handed_over"]:
                line += "  (%d points handed over)" % d["handed_over"]
        print(line)
    print("  %-8s %6d windows %6.2f %%" % ("rejected", s["rejected"]["windows"], 100.0 * s["rejected"]["windows"] / max(tot, 1)))
    print("  every accepted eccentric window: tiered bodies %.3e km %.3e km/s, general body throughout %.3e km %.3e km/s" % (
        s["all"]["own"] + s["all"]["general"]))


if __name__ == "__main__":
    from astroz_amd import synth
    from oracle import oracle
    oracle.build()
    n_sats = int(sys.argv[1]) if len(sys.argv) > 1 else 13478
    n_times = int(sys.argv[2]) if len(sys.argv) > 2 else 1440
    tile_e = int(sys.argv[3]) if len(sys.argv) > 3 else 768  # (beside a bulk four times their number the eccentric rows take its segments)
    seed = int(sys.argv[4]) if len(sys.argv) > 4 else 20260926
    pairs = synth.synth_catalog(n_near=n_sats, n_deep=0, seed=seed)
    res = run(load(), oracle, pairs, np.arange(n_times, dtype=np.float64), lambda ep: (synth.START_JD - ep) * 1440.0, tile_e,
              threads=min(os.cpu_count() or 1, 16))
    report(summarize(res, tile_e), "%d satellites (%d eccentric rows) x %d one-minute steps, eccentric segments of %d" % (
        n_sats, len(res["idx"]), n_times, tile_e))
