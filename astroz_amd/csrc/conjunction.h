// conjunction.h -- the closest approach of two objects inside one grid interval: the model of the conjunction finder
// (azh_find_conjunctions_*), one source for the kernel and for its host twin (azh_closest_approach).  Included by
// astroz_hip.hip after devmath.h.
//
// For a catalog member s and a target t, d = r_s - r_t and w = v_s - v_t (TEME, km and km/s) and q = d.w, half the rate of
// |d|^2.  A grid interval [t0, t1] of dt minutes is a BRACKET when q0 < 0 and q1 >= 0: the distance falls at its left end and
// no longer falls at its right end, so a minimum lies inside.  On a bracket the relative track is the cubic Hermite interpolant
// of d, component by component, with the end slopes m = 60 dt w (km per unit of sigma), in the monomial form
//     d(sigma) = d0 + sigma (m0 + sigma (c2 + sigma c3)),   D = d1 - d0,   c2 = 3 D - 2 m0 - m1,   c3 = m0 + m1 - 2 D
// and the closest approach is the root in [0, 1] of f(sigma) = d(sigma).d'(sigma): f(0) = 60 dt q0 < 0 <= 60 dt q1 = f(1), so
// the root is bracketed by construction.  It is found by regula falsi with the Illinois correction (az_culmination's
// iteration) from the secant of the ends: f is a quintic whose evaluation costs 21 multiply-adds, and a straight relative
// track -- f linear -- is solved by the first step.  Then
//     t_tca = t0 + sigma dt,   miss = |d(sigma)|,   relative speed = |d'(sigma)| / (60 dt).
//
// The distance bound of az_ca_far (the kernel's prefilter; it must never lose an event).  With a = m0 - D and b = m1 - D the
// Hermite is the chord plus a bounded bend,
//     d(sigma) = d0 + sigma D + e(sigma),   e = sigma (1 - sigma)^2 a - sigma^2 (1 - sigma) b,
//     |e| <= sigma (1 - sigma) ((1 - sigma) |a| + sigma |b|) <= max(|a|, |b|) / 4,
// so |d(sigma)| >= (distance from the origin to the chord SEGMENT d0-d1) - max(|a|, |b|) / 4 on the whole interval: a bracket
// whose chord stays further than threshold + max(|a|, |b|) / 4 from the origin cannot hold a miss below the threshold.  The
// bound is one on the interpolant itself, which is what defines the event; it is not an estimate of the true orbit's
// curvature.  (For two low orbits over a minute |a| is the relative acceleration times 1,800 s^2, up to ~30 km.)  The comparison
// carries a relative slack of 1e-12 against the rounding of its own few operations.
//
// Not modelled: light time, covariance, probability of collision.
#pragma once
#include <math.h>

struct AzApproach {
    double sigma, miss, speed; // place in [0, 1]; km; km/s
};

__host__ __device__ inline double az_ca_dot(const double a[3], const double b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// q0 = d0.w0, q1 = d1.w1 (NaN is no bracket)
__host__ __device__ inline bool az_ca_bracket(double q0, double q1) { return q0 < 0.0 && q1 >= 0.0; }

// the prefilter: true when the bracket cannot hold a miss below threshold_km (the bound above)
__host__ __device__ inline bool az_ca_far(const double d0[3], const double w0[3], const double d1[3], const double w1[3], double dt_min,
                                          double threshold_km)
{
    const double k = 60.0 * dt_min;
    double D[3], a2 = 0.0, b2 = 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        D[j] = d1[j] - d0[j];
        const double a = k * w0[j] - D[j], b = k * w1[j] - D[j];
        a2 += a * a;
        b2 += b * b;
    }
    const double DD = az_ca_dot(D, D), p = -az_ca_dot(d0, D);
    const double tau = DD > 0.0 ? fmin(fmax(p / DD, 0.0), 1.0) : 0.0; // the chord's point nearest to the origin
    const double c[3] = {d0[0] + tau * D[0], d0[1] + tau * D[1], d0[2] + tau * D[2]};
    const double reach = (threshold_km + 0.25 * sqrt(fmax(a2, b2))) * (1.0 + 1.0e-12);
    return az_ca_dot(c, c) > reach * reach;
}

// the closest approach on a bracket (the caller has checked az_ca_bracket)
__host__ __device__ inline AzApproach az_ca_refine(const double d0[3], const double w0[3], const double d1[3], const double w1[3],
                                                   double dt_min)
{
    const double k = 60.0 * dt_min;
    double m0[3], c2[3], c3[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double D = d1[j] - d0[j], m1 = k * w1[j];
        m0[j] = k * w0[j];
        c2[j] = 3.0 * D - 2.0 * m0[j] - m1;
        c3[j] = m0[j] + m1 - 2.0 * D;
    }
    double x[3], xd[3];
    auto track = [&](double s) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            x[j] = d0[j] + s * (m0[j] + s * (c2[j] + s * c3[j]));
            xd[j] = m0[j] + s * (2.0 * c2[j] + s * (3.0 * c3[j]));
        }
    };
    auto f = [&](double s) {
        track(s);
        return az_ca_dot(x, xd);
    };
    double lo = 0.0, hi = 1.0, g_lo = f(0.0), g_hi = f(1.0), s = 1.0;
    if (!(g_lo < 0.0)) { // (q0 < 0 within the rounding of the slopes' scaling: the minimum is the left end)
        s = 0.0;
    } else if (g_hi > 0.0) { // (g_hi == 0: the minimum is the right end)
        int side = 0;
        s = 0.5;
        for (int it = 0; it < 60; ++it) {
            const double sn = (lo * g_hi - hi * g_lo) / (g_hi - g_lo);
            const bool done = fabs(sn - s) <= 1.0e-15;
            s = sn;
            const double gs = f(s);
            if (done || gs == 0.0) break;
            if (gs < 0.0) {
                lo = s; g_lo = gs;
                if (side == 1) g_hi *= 0.5;
                side = 1;
            } else {
                hi = s; g_hi = gs;
                if (side == -1) g_lo *= 0.5;
                side = -1;
            }
        }
    }
    track(s);
    AzApproach o;
    o.sigma = s;
    o.miss = sqrt(az_ca_dot(x, x));
    o.speed = sqrt(az_ca_dot(xd, xd)) / k;
    return o;
}
