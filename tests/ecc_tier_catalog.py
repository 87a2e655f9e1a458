"""Hand-built catalog for the tests of the eccentric loop bodies of k_rows_fast (not a test module): near-earth element
sets from synth.format_tle whose eccentricities straddle every boundary the eccentric form knows -- the classes (0.0025,
0.0075, 0.1), the bound of body E1 (el <= 0.01, where el exceeds the eccentricity by up to ~0.0011 sin i) and of body E2
(el <= 0.1) -- up to 0.25, each with low- and high-drag members, epochs 0 to 5 days before the grid and several
inclinations, and two members whose windows the plan rejects."""
import numpy as np

from astroz_amd import synth

ECCS = (0.0024, 0.0026, 0.0074, 0.0076, 0.0084, 0.0106, 0.0975, 0.1005, 0.2, 0.25)
# (epoch days before START_JD, inclination, bstar, perigee altitude km)
MEMBERS = ((0.0, 28.5, 1.0e-5, 520.0), (1.0, 51.6, 2.0e-4, 460.0), (2.5, 63.4, 5.0e-4, 400.0), (5.0, 98.0, 3.0e-5, 600.0))


def _mm(alt_km, ecc):
    """rev/day for a perigee altitude (km) and eccentricity (WGS-72)."""
    a = (1.0 + alt_km / 6378.135) / (1.0 - ecc)
    return 0.0743669161331734132 / a ** 1.5 * 1440.0 / (2.0 * np.pi)


def ecc_rows():
    rows = []  # (epoch days before START_JD, incl, raan, ecc, argp, ma, perigee altitude km, bstar)
    for k, ecc in enumerate(ECCS):
        for j, (days, incl, bstar, alt) in enumerate(MEMBERS):
            rows.append((days, incl, 25.0 * k + 7.0 * j, ecc, 300.0 - 33.0 * k + 80.0 * j, 15.0 + 47.0 * k + 90.0 * j, alt + 10.0 * k, bstar))
    # windows the plan rejects: very high drag on a low perigee, days from epoch (the drag series leave their bounds) -- one
    # member rejected throughout, two that leave the bounds in the course of a day (after E1 / the general body)
    rows.append((5.0, 51.6, 200.0, 0.03, 130.0, 310.0, 230.0, 5.0e-3))
    rows.append((3.0, 51.6, 210.0, 0.005, 130.0, 310.0, 300.0, 5.0e-3))
    rows.append((5.0, 51.6, 220.0, 0.15, 130.0, 310.0, 230.0, 1.0e-2))
    # as eccentric as a near-earth period (< 225 min) allows: the general body hands over where Newton needs a wider first trip
    rows.append((0.5, 40.0, 120.0, 0.42, 200.0, 30.0, 300.0, 2.0e-5))
    return rows


def ecc_pairs():
    return [synth.format_tle(71001 + i, synth.START_JD - days, incl, raan % 360.0, ecc, argp % 360.0, ma % 360.0, _mm(alt, ecc), bstar)
            for i, (days, incl, raan, ecc, argp, ma, alt, bstar) in enumerate(ecc_rows())]


def filler_pairs(n=200):
    """Near-circular members (class 0) to put beside the catalog on the GPU: with at least four times as many of them as
    eccentric rows, the eccentric launch takes the bulk's segment length, a forced one included."""
    return [synth.format_tle(73001 + i, synth.START_JD - 0.1 * (i % 30), 30.0 + 0.4 * i, (11.0 * i) % 360.0, 0.0003 + 0.00001 * (i % 100),
                             (37.0 * i) % 360.0, (53.0 * i) % 360.0, _mm(500.0 + 2.0 * i, 0.001), 2.0e-5) for i in range(n)]


def jdfr_times(n, epochs, start_jd=None):
    """A (jd, fr) grid of one-minute steps as the reference's Python API builds it: times and per-satellite offsets."""
    start_jd = synth.START_JD if start_jd is None else start_jd
    jd = np.full(n, start_jd)
    fr = 0.32853009 + np.arange(n) / 1440.0
    ref = jd[0] + fr[0]
    return ((jd + fr) - ref) * 1440.0, (ref - epochs) * 1440.0
