// los.h -- line of sight between two objects past a spherical Earth: the geometry of the access finder (azh_find_access_*),
// one source for the kernel and for its host twin (azh_line_of_sight).  Included by astroz_hip.hip after devmath.h.
//
// For two TEME positions r1 (a catalog member) and r2 (the target), d = r2 - r1, and an Earth of radius R = 6378.137 km:
// `clearance` is the distance from the Earth's centre to the SEGMENT r1-r2.  With tau = -r1.d / |d|^2 the parameter of the
// point of the line closest to the centre, it is |r1 x r2| / |d| when 0 < tau < 1 -- the cross-product form, which has none of
// the cancellation of sqrt(|r|^2 - x^2) -- and |r1| (tau <= 0, or |d| = 0) or |r2| (tau >= 1) otherwise.  The cross product is
// taken as r1 x d, the same vector: its rounding error scales with |r1| |d| like the divisor, so two objects a metre apart keep
// a clearance good to an ulp of |r1|, where the ulp of |r1| |r2| over |d| would be metres.
//     g = clearance - (R + grazing altitude)                                    no range limit
//     g = min(clearance - (R + grazing altitude), max range - |d|)              with one
// and the two objects have access to each other when g >= 0.  The rates of the two margins follow from r1, v1, r2, v2, that of
// the clearance on the branch that is active (as eclipse_kernel.h does for max(f, -x)).  Not modelled: the Earth's oblateness,
// atmospheric refraction, light time.
#pragma once

#define AZ_LOS_R_EARTH 6378.137

struct AzLos {
    double clearance, range; // km
    int branch;              // where the segment is closest to the centre: 0 at r1, 1 inside, 2 at r2
};
// rsqrt(x) = 1 / sqrt(x)
template <class Rsqrt>
__host__ __device__ inline AzLos az_los(const double r1[3], const double r2[3], Rsqrt &&rsqrt)
{
    const double d[3] = {r2[0] - r1[0], r2[1] - r1[1], r2[2] - r1[2]};
    const double d2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    const double q = -(r1[0] * d[0] + r1[1] * d[1] + r1[2] * d[2]); // tau |d|^2
    const double id = d2 > 0.0 ? rsqrt(d2) : 0.0;
    AzLos o;
    o.range = d2 * id;
    if (q > 0.0 && q < d2) {
        const double cx = r1[1] * d[2] - r1[2] * d[1], cy = r1[2] * d[0] - r1[0] * d[2], cz = r1[0] * d[1] - r1[1] * d[0];
        const double c2 = cx * cx + cy * cy + cz * cz;
        o.clearance = c2 > 0.0 ? (c2 * rsqrt(c2)) * id : 0.0;
        o.branch = 1;
    } else {
        const bool far = q > 0.0; // (|d| = 0: q = 0, r1)
        const double e0 = far ? r2[0] : r1[0], e1 = far ? r2[1] : r1[1], e2c = far ? r2[2] : r1[2];
        const double e2 = e0 * e0 + e1 * e1 + e2c * e2c;
        o.clearance = e2 > 0.0 ? e2 * rsqrt(e2) : 0.0;
        o.branch = far ? 2 : 0;
    }
    return o;
}

// the two margins whose minimum is g, and their rates (km/s), for the states (r1, v1), (r2, v2): gc = clearance - r_graze
// (r_graze = R + grazing altitude) with its rate on the branch of the clearance that is active, gr = max_range - |d|
// (max_range = +infinity for no limit: gr = +infinity, rate 0)
struct AzLosMargins {
    double gc, gcd, gr, grd;
};
template <class Rsqrt>
__host__ __device__ inline AzLosMargins az_los_margins(const double r1[3], const double v1[3], const double r2[3], const double v2[3],
                                                       double r_graze, double max_range, Rsqrt &&rsqrt)
{
    const AzLos o = az_los(r1, r2, rsqrt);
    const double d[3] = {r2[0] - r1[0], r2[1] - r1[1], r2[2] - r1[2]}, w[3] = {v2[0] - v1[0], v2[1] - v1[1], v2[2] - v1[2]};
    const double dw = d[0] * w[0] + d[1] * w[1] + d[2] * w[2];
    AzLosMargins m;
    m.gc = o.clearance - r_graze;
    m.gr = max_range - o.range;
    m.grd = o.range > 0.0 ? -dw / o.range : 0.0;
    if (o.branch == 1) {
        // c = |n| / |d|, n = r1 x d:  c' = n.n' / (|n| |d|) - c d.d' / |d|^2,  n' = v1 x d + r1 x d'
        const double n[3] = {r1[1] * d[2] - r1[2] * d[1], r1[2] * d[0] - r1[0] * d[2], r1[0] * d[1] - r1[1] * d[0]};
        const double nd[3] = {v1[1] * d[2] - v1[2] * d[1] + r1[1] * w[2] - r1[2] * w[1], v1[2] * d[0] - v1[0] * d[2] + r1[2] * w[0] - r1[0] * w[2],
                              v1[0] * d[1] - v1[1] * d[0] + r1[0] * w[1] - r1[1] * w[0]};
        const double nn = n[0] * nd[0] + n[1] * nd[1] + n[2] * nd[2];
        const double ir = 1.0 / o.range; // (branch 1: |d| > 0)
        m.gcd = o.clearance > 0.0 ? (nn * ir * ir) / o.clearance - o.clearance * dw * ir * ir : 0.0;
    } else {
        const double rv1 = r1[0] * v1[0] + r1[1] * v1[1] + r1[2] * v1[2], rv2 = r2[0] * v2[0] + r2[1] * v2[1] + r2[2] * v2[2];
        m.gcd = o.clearance > 0.0 ? (o.branch == 2 ? rv2 : rv1) / o.clearance : 0.0;
    }
    return m;
}
