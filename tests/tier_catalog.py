"""Hand-built catalog for the tests of k_rows_fast's tiered loop bodies (not a test module): about 40 element sets from
synth.format_tle chosen so that the window plan assigns every body tier, with members on both sides of every eccentricity
threshold the fast step knows."""
import numpy as np

from astroz_amd import synth


def _mm(alt_km, ecc):
    """rev/day for a perigee altitude (km) and eccentricity (WGS-72)."""
    a = (1.0 + alt_km / 6378.135) / (1.0 - ecc)
    return 0.0743669161331734132 / a ** 1.5 * 1440.0 / (2.0 * np.pi)


def tier_pairs():
    rows = []  # (epoch days before START_JD, incl, raan, ecc, argp, ma, perigee altitude km, bstar)
    # low drag, near-circular, fresh elements: every inclination band (the eps tier)
    for k, incl in enumerate((0.5, 5.0, 28.5, 43.0, 53.0, 70.0, 86.4, 97.6, 116.0, 144.0)):
        rows.append((0.3 + 0.05 * k, incl, 20.0 * k, 0.0002 + 0.0001 * k, 35.0 * k, 50.0 * k, 540.0 + 12.0 * k, 2.0e-5))
    # low, equatorial, fast node
    for k, (alt, incl) in enumerate(((230.0, 0.2), (260.0, 3.0), (300.0, 1.0), (340.0, 8.0))):
        rows.append((0.2, incl, 10.0 + k, 0.0004, 80.0, 200.0 + k, alt, 1.0e-5))
    for k, (alt, incl) in enumerate(((150.0, 0.2), (160.0, 0.3), (180.0, 179.6), (195.0, 0.4))):
        rows.append((0.05, incl, 40.0 + k, 0.0005, 60.0, 20.0 + k, alt, 1.0e-6))
    # high drag, several days from epoch: the general body (the along-track drag phase leaves the 2^-10 tier)
    for k, (days, alt, bstar) in enumerate(((5.0, 300.0, 8.0e-4), (7.0, 320.0, 1.2e-3), (9.0, 280.0, 5.0e-4), (6.0, 350.0, 2.0e-3),
                                            (12.0, 400.0, 1.5e-3), (4.0, 260.0, 1.0e-3))):
        rows.append((days, 51.6 + k, 30.0 * k, 0.0006 + 0.0002 * k, 60.0 * k, 100.0 + 40.0 * k, alt, bstar))
    # the eccentricity thresholds: 0.0025 (near-circular / eccentric form), 0.0075, 0.1 (classes), and beyond
    for k, ecc in enumerate((0.0024, 0.0026, 0.0074, 0.0076, 0.02, 0.099, 0.101, 0.2)):
        for days, incl in ((0.4, 63.4), (3.0, 98.0)):
            rows.append((days, incl, 15.0 * k, ecc, 270.0 - 20.0 * k, 10.0 + 30.0 * k, 450.0 + 40.0 * k, 5.0e-5))
    # perigee below 220 km (the simplified-drag flag), near-circular and eccentric
    rows.append((0.5, 51.6, 200.0, 0.0008, 120.0, 300.0, 205.0, 3.0e-5))
    rows.append((0.5, 65.0, 210.0, 0.03, 130.0, 310.0, 190.0, 3.0e-5))
    # nearly zero eccentricity: the lower bound on em decides (the step carries no clamp)
    rows.append((0.3, 53.0, 100.0, 0.0000012, 0.0, 0.0, 550.0, 1.0e-4))
    rows.append((2.0, 53.0, 110.0, 0.0000100, 0.0, 90.0, 550.0, 2.0e-4))
    pairs = []
    for i, (days, incl, raan, ecc, argp, ma, alt, bstar) in enumerate(rows):
        pairs.append(synth.format_tle(70001 + i, synth.START_JD - days, incl, raan % 360.0, ecc, argp % 360.0, ma % 360.0,
                                      _mm(alt, ecc), bstar))
    return pairs


def jdfr_times(n, epochs, start_jd=None):
    """A (jd, fr) grid of one-minute steps as the reference's Python API builds it: times and per-satellite offsets."""
    start_jd = synth.START_JD if start_jd is None else start_jd
    jd = np.full(n, start_jd)
    fr = 0.32853009 + np.arange(n) / 1440.0
    ref = jd[0] + fr[0]
    return ((jd + fr) - ref) * 1440.0, (ref - epochs) * 1440.0
