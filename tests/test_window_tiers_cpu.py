"""CPU tier: the tiered loop bodies of k_rows_fast (fast_step.h AZ_TIER_*), host-compiled by tests/host_emul/emul_tiers.cpp.

The window plan gives every (satellite, time segment) window of the near-circular form a body tier from rigorous bounds on
the widest small rotation of the step (eps, the rest of the along-track phase); the row kernel runs the loop body compiled
for that tier.  Checked here, one row at a time as the kernel runs it:
  * the catalog makes the plan assign every tier, on every shape;
  * every body matches the oracle on the windows the plan gives it, at the gates of tests/test_gpu_parity.py;
  * no bound is violated: the bounded quantities, evaluated at EVERY grid point of such a window, stay inside the tier's bound
    (and em stays above the floor the step no longer clamps at);
  * the general body gives the same results on the windows of the eps tier (asserted against the oracle gates).
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tier_catalog  # noqa: E402

TOL_R = 1e-6   # km    (tests/test_gpu_parity.py)
TOL_V = 1e-9   # km/s
GENERAL, EPS = 0, 1
EPS_MAX = 2.0 ** -10      # AZ_TIER_EPS_MAX
ROT_MED = 0.125           # bound on eps and a_nd of every accepted window
ROT_16TH = 0.0625         # bound on th
EM_MIN = 1.0e-6           # AZ_FAST_EM_MIN
DELTA_MAX = 4.0e-6        # AZ_DELTA_MAX
P_TH, P_EM, P_EPS, P_ND = range(4)
# (name, grid points, segment of the near-circular form, segment of the eccentric form, (jd, fr) grid)
SHAPES = (("two_windows", 200, 128, 128, False), ("day", 1440, 768, 256, False), ("jdfr", 200, 128, 128, True))


@pytest.fixture(scope="module")
def emul_tiers(tmp_path_factory):
    src = os.path.join(ROOT, "tests", "host_emul", "emul_tiers.cpp")
    lib = str(tmp_path_factory.mktemp("emul_tiers") / "libemul_tiers.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wno-unknown-pragmas", "-o", lib, src])
    E = C.CDLL(lib)
    E.emul_tiers_init.restype = C.c_uint
    E.emul_tiers_init.argtypes = [C.c_void_p] * 3
    E.emul_tiers_row.restype = None
    E.emul_tiers_row.argtypes = [C.c_void_p, C.c_uint, C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int,
                                 C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
    assert E.emul_tiers_num_probes() == 4
    return E


@pytest.fixture(scope="module")
def runs(emul_tiers, orc):
    """Per shape: the oracle's rows, and the emulated rows through each window's own body and through the general body."""
    from astroz_amd import synth
    E = emul_tiers
    pairs = tier_catalog.tier_pairs() + synth.synth_catalog(n_near=160, n_deep=0, seed=77)
    tles = [orc.parse_lines(a, b) for a, b in pairs]
    cat = orc.Catalog(tles, 1)
    g = np.array([6378.135, 0.001082616, -0.00000165597, 0.0743669161331734132, -0.00234506972242078,
                  0.0743669161331734132 * 6378.135 / 60.0])
    nf = E.emul_tiers_num_fields()
    out = {}
    for name, n, tile_c, tile_e, jdfr in SHAPES:
        if jdfr:
            times, off = tier_catalog.jdfr_times(n, cat.epoch_jd)
        else:
            times, off = np.arange(n, dtype=np.float64), (synth.START_JD - cat.epoch_jd) * 1440.0
        step = (times[-1] - times[0]) / (n - 1)
        delta = (times - (times[0] + np.arange(n) * step)).astype(np.float32)
        assert np.abs(delta).max() <= DELTA_MAX and (jdfr or not delta.any())
        _, p0, v0 = cat.propagate(times, off, layout=orc.SAT_MAJOR)
        res = {"p0": p0, "v0": v0, "ecc": np.zeros(len(tles), dtype=bool)}
        for key, force in (("own", -1), ("general", GENERAL)):
            o = np.full((len(tles), n, 6), np.nan)
            tier = np.zeros((len(tles), n), dtype=np.int32)
            probe = np.zeros((len(tles), n, 4))
            for i, t in enumerate(tles):
                raw = np.array([t.epoch_jd, t.mm_revday, t.ecc, t.incl_deg, t.raan_deg, t.argp_deg, t.ma_deg, t.bstar])
                fields = np.zeros(nf)
                flags = E.emul_tiers_init(raw.ctypes.data, g.ctypes.data, fields.ctypes.data)
                assert (flags & 0x1ff) == 0
                ecc = 1 if ((flags >> 12) & 3) else 0
                res["ecc"][i] = bool(ecc)
                E.emul_tiers_row(fields.ctypes.data, flags, g.ctypes.data, times[0] + off[i], step, n, tile_e if ecc else tile_c, ecc,
                                 force, delta.ctypes.data if jdfr else None, DELTA_MAX if jdfr else 0.0,
                                 o[i].ctypes.data, tier[i].ctypes.data, probe[i].ctypes.data)
            res[key] = (o, tier, probe)
        out[name] = res
    return out


def _sel(res, tier_value):
    """Grid points of near-circular rows whose window carries tier_value."""
    return (res["own"][1] == tier_value) & ~res["ecc"][:, None]


@pytest.mark.parametrize("shape", [s[0] for s in SHAPES])
def test_plan_assigns_every_tier(runs, shape):
    res = runs[shape]
    for tier_value in (GENERAL, EPS):
        assert _sel(res, tier_value).any(), "no window of tier %d on shape %s" % (tier_value, shape)
    assert (res["own"][1] == -1).any()                       # ... and some windows go to the generic step
    assert (res["own"][1][res["ecc"]] == GENERAL).any()      # the eccentric form runs too
    # both sides of the near-circular threshold, the lower bound on em included
    assert (res["own"][1] == -1)[~res["ecc"]].any() and (res["own"][1] >= 0)[~res["ecc"]].any()


@pytest.mark.parametrize("shape", [s[0] for s in SHAPES])
def test_every_body_matches_the_oracle_on_its_windows(runs, shape):
    res = runs[shape]
    o, tier, _ = res["own"]
    for label, sel in (("general", _sel(res, GENERAL)), ("eps", _sel(res, EPS)),
                       ("eccentric", (tier >= 0) & res["ecc"][:, None])):
        dr = float(np.abs(o[sel][:, :3] - res["p0"][sel]).max())
        dv = float(np.abs(o[sel][:, 3:] - res["v0"][sel]).max())
        print("%s %-9s %7d points  max|dr| = %.3e km  max|dv| = %.3e km/s" % (shape, label, int(sel.sum()), dr, dv))
        assert dr < TOL_R and dv < TOL_V, (shape, label, dr, dv)


@pytest.mark.parametrize("shape", [s[0] for s in SHAPES])
def test_no_tier_bound_is_violated_at_any_grid_point(runs, shape):
    res = runs[shape]
    _, tier, probe = res["own"]
    ok = tier >= 0
    assert np.abs(probe[ok][:, P_TH]).max() <= ROT_16TH
    assert np.abs(probe[ok][:, P_EPS]).max() <= ROT_MED and np.abs(probe[ok][:, P_ND]).max() <= ROT_MED
    assert probe[ok][:, P_EM].min() >= EM_MIN
    eps_max = float(np.abs(probe[_sel(res, EPS)][:, P_EPS]).max())
    print("%s: largest |eps| on eps-tier windows %.3e (bound %.3e)" % (shape, eps_max, EPS_MAX))
    assert eps_max <= EPS_MAX
    # the split is worth having: windows of the general tier do leave the eps tier's bound
    gen = _sel(res, GENERAL)
    assert np.abs(probe[gen][:, P_EPS]).max() > EPS_MAX


@pytest.mark.parametrize("shape", [s[0] for s in SHAPES])
def test_general_body_agrees_on_the_eps_tiers_windows(runs, shape):
    res = runs[shape]
    o, _, _ = res["own"]
    og, tier_g, _ = res["general"]
    assert np.array_equal(tier_g, res["own"][1])
    sel = _sel(res, EPS)
    dr = float(np.abs(og[sel][:, :3] - res["p0"][sel]).max())
    dv = float(np.abs(og[sel][:, 3:] - res["v0"][sel]).max())
    assert dr < TOL_R and dv < TOL_V, (shape, dr, dv)
    diff_r = float(np.abs(og[sel][:, :3] - o[sel][:, :3]).max())
    diff_v = float(np.abs(og[sel][:, 3:] - o[sel][:, 3:]).max())
    print("%s: general body vs eps body on %d points: max|dr| = %.3e km, max|dv| = %.3e km/s" % (shape, int(sel.sum()), diff_r, diff_v))
    # the dropped term: eps^4/24 < 3.8e-14 rad of a rotation of a vector of < 1e4 km / 8 km/s, plus a few roundings -- three orders of magnitude inside the gates, which are what is asserted
    assert diff_r < TOL_R and diff_v < TOL_V
