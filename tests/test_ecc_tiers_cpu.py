"""CPU tier: the loop bodies of k_rows_fast's eccentric form (fast_step.h AZ_ETIER_*), host-compiled by
tests/host_emul/emul_ecc_tiers.cpp and driven through tools/ecc_tier_study.py.

The window plan gives every accepted (satellite, time segment) window of the eccentric form a body from its rigorous upper
bound on el: E1 (el <= 0.01: the near-circular Kepler form, one notch wider), E2 (el <= 0.1: three Newton trips with fixed
rotation tiers) or the general five-trip body with its per-step predicate.  Checked here, one row at a time as the kernel runs it:
  * the hand-built catalog (tests/ecc_tier_catalog.py) makes the plan assign every body at least five windows and reject at
    least two, on every shape;
  * every body matches the oracle on the windows the plan gives it at the gates of tests/test_gpu_parity.py, and so does the
    general body on the same windows, and the two agree at the same gates;
  * at EVERY grid point of a window of E1 or E2 the quantities the derivations beside AZ_ETIER_E1 / AZ_ETIER_E2 bound stay
    inside those bounds: el, each correction of the Kepler iteration, the generic loop's exit criterion el^2 d^4 < 4e-26 --
    and neither body ever raises the Newton predicate;
  * over every eccentric row of the headline catalog (13,478 satellites, a day of one-minute steps) the tiered bodies' worst
    difference from the oracle is at most twice that of the general body on the same rows in the same run.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ecc_tier_catalog  # noqa: E402
import ecc_tier_study as study  # noqa: E402

TOL_R = 1e-6   # km    (tests/test_gpu_parity.py)
TOL_V = 1e-9   # km/s
GENERAL, E1, E2 = 0, 1, 2
E1_MAX, E2_MAX = 0.01, 0.1   # AZ_ETIER_E1_MAX, AZ_ETIER_E2_MAX
ROT_MED = 0.125              # az_pq_med: trip 0 of E2
ROT_MILLI = 0.0041           # az_fpq_milli: trip 1 of E2
ROT_16TH = 0.0625            # bound on th
EM_MIN = 1.0e-6              # AZ_FAST_EM_MIN
P = {name: k for k, name in enumerate(study.PROBES)}
# (name, grid points, segment of the eccentric form, (jd, fr) grid)
SHAPES = (("two_windows", 200, 128, False), ("day", 1440, 256, False), ("jdfr", 200, 128, True))


def _bounds(el):
    """Bounds on |d0|, |d1|, |d2| of body E1 / E2 from the window's bound on el (fast_step.h, beside AZ_ETIER_*).
    Newton from E0 = u: |E* - E0| <= el, |d0| <= el/(1 - el), error after a Newton trip e' <= el e^2 / (2 (1 - el));
    a chord step with trip 0's reciprocal leaves e' <= e el^2/(1 - el)^2.  A correction is the difference of two errors."""
    d0 = el / (1.0 - el)
    e1 = el ** 3 / (2.0 * (1.0 - el))
    if el <= E1_MAX:       # E1: Newton, chord, chord
        e2 = e1 * el ** 2 / (1.0 - el) ** 2
        e3 = e2 * el ** 2 / (1.0 - el) ** 2
    else:                  # E2: three Newton trips
        e2 = el * e1 ** 2 / (2.0 * (1.0 - el))
        e3 = el * e2 ** 2 / (2.0 * (1.0 - el))
    return d0, e1 + e2, e2 + e3


@pytest.fixture(scope="module")
def emul_ecc(tmp_path_factory):
    return study.load(str(tmp_path_factory.mktemp("emul_ecc_tiers")))


@pytest.fixture(scope="module")
def runs(emul_ecc, orc):
    from astroz_amd import synth
    pairs = ecc_tier_catalog.ecc_pairs()
    out = {}
    for name, n, tile, jdfr in SHAPES:
        if jdfr:
            times = ecc_tier_catalog.jdfr_times(n, np.zeros(1))[0]
            off = lambda ep, n=n: ecc_tier_catalog.jdfr_times(n, ep)[1]  # noqa: E731
        else:
            times = np.arange(n, dtype=np.float64)
            off = lambda ep: (synth.START_JD - ep) * 1440.0  # noqa: E731
        res = study.run(emul_ecc, orc, pairs, times, off, tile, quasi=jdfr)
        res["summary"] = study.summarize(res, tile)
        study.report(res["summary"], "%s: %d eccentric rows x %d steps, segments of %d" % (name, len(res["idx"]), n, tile))
        out[name] = res
    return out


@pytest.mark.parametrize("shape", [s[0] for s in SHAPES])
def test_plan_assigns_every_body(runs, shape):
    s = runs[shape]["summary"]
    # a condition on the catalog, not a measurement: with fewer windows the tests below prove nothing about a body
    for name in ("E1", "E2", "general"):
        assert s[name]["windows"] >= 5, (shape, name, s[name]["windows"])
    assert s["rejected"]["windows"] >= 2, (shape, s["rejected"])
    # members on both sides of either bound, and the class-0 members of the catalog are not part of the eccentric form
    assert len(runs[shape]["idx"]) == len(ecc_tier_catalog.ecc_pairs()) - 4


@pytest.mark.parametrize("shape", [s[0] for s in SHAPES])
def test_every_body_matches_the_oracle_and_the_general_body(runs, shape):
    s = runs[shape]["summary"]
    for name in ("E1", "E2", "general"):
        d = s[name]
        print("%s %-8s %6d points: vs oracle %.3e km %.3e km/s; general body on the same windows %.3e km %.3e km/s; between them "
              "%.3e km %.3e km/s" % ((shape, name, d["points"]) + d["own"] + d["general"] + d["cross"]))
        for key in ("own", "general", "cross"):
            assert d[key][0] < TOL_R and d[key][1] < TOL_V, (shape, name, key, d[key])
    # E1 and E2 are proven from the window's bound: no point of theirs is handed over
    assert s["E1"]["handed_over"] == 0 and s["E2"]["handed_over"] == 0


@pytest.mark.parametrize("shape", [s[0] for s in SHAPES])
def test_no_bound_is_violated_at_any_grid_point(runs, shape):
    res = runs[shape]
    tier = res["tier"]
    _, bad, probe = res["own"]
    ok = tier >= 0
    assert np.abs(probe[ok][:, P["th"]]).max() <= ROT_16TH
    assert np.abs(probe[ok][:, P["eps"]]).max() <= ROT_MED and np.abs(probe[ok][:, P["a_nd"]]).max() <= ROT_MED
    assert probe[ok][:, P["em"]].min() >= EM_MIN
    for v, name, el_max in ((E1, "E1", E1_MAX), (E2, "E2", E2_MAX)):
        q = probe[tier == v]
        assert not bad[tier == v].any()
        el = np.sqrt(q[:, P["el2"]])
        d0, d1, d2 = (np.abs(q[:, P[k]]) for k in ("d0", "d1", "d2"))
        b0, b1, b2 = _bounds(el_max)
        exit_crit = q[:, P["el2"]] * d2 ** 4
        print("%s %s: el <= %.4e (%.2g)  |d0| <= %.3e (%.3e)  |d1| <= %.3e (%.3e)  |d2| <= %.3e (%.3e)  el^2 d2^4 <= %.3e (4e-26)" % (
            shape, name, el.max(), el_max, d0.max(), b0, d1.max(), b1, d2.max(), b2, exit_crit.max()))
        assert el.max() <= el_max
        assert d0.max() <= b0 and d1.max() <= b1 and d2.max() <= b2
        assert exit_crit.max() < 4.0e-26
        if v == E2:  # the fixed rotation tiers of its trips
            assert b0 <= ROT_MED and b1 <= ROT_MILLI
    # the split is worth having: windows on the far side of either bound exist and do leave it
    assert np.sqrt(probe[tier == E2][:, P["el2"]]).max() > E1_MAX
    g = res["general"][2]
    assert np.sqrt(g[tier == GENERAL][:, P["el2"]]).max() > E2_MAX


def test_headline_catalog_tiered_bodies_within_twice_the_general_body(emul_ecc, orc):
    """Every eccentric row of the headline workload, all 1,440 steps, both measured in this run."""
    from astroz_amd import synth
    pairs = synth.synth_catalog(n_near=13478, n_deep=0, seed=20260926)
    res = study.run(emul_ecc, orc, pairs, np.arange(1440, dtype=np.float64), lambda ep: (synth.START_JD - ep) * 1440.0, 768,
                    threads=min(os.cpu_count() or 1, 16))
    s = study.summarize(res, 768)  # (the segment length the library gives the eccentric rows of this catalog)
    study.report(s, "headline catalog: %d eccentric rows x 1440 steps, segments of 768" % len(res["idx"]))
    assert s["E1"]["windows"] > 0 and s["E2"]["windows"] > 0 and s["general"]["windows"] > 0
    (r_own, v_own), (r_gen, v_gen) = s["all"]["own"], s["all"]["general"]
    assert r_gen < TOL_R and v_gen < TOL_V
    assert r_own <= 2.0 * r_gen and v_own <= 2.0 * v_gen, (r_own, v_own, r_gen, v_gen)
