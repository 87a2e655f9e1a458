// sun.h -- the Sun's position and the Earth-shadow function of the eclipse finder (azh_find_eclipses_*), one source for the
// kernels and for their host twins (azh_sun_position_teme, azh_shadow_state).  Included by astroz_hip.hip after devmath.h.
//
// Sun: the low-precision solar position of the Astronomical Almanac as Vallado gives it (Fundamentals of Astrodynamics and
// Applications, algorithm "Sun"), stated accuracy 0.01 degrees between 1950 and 2050.  Two simplifications, both below that
// figure: the Julian date is taken as it comes (UTC; UT1 and TT, which the two series want, differ from it by about a minute,
// 1e-5 degrees of solar longitude), and the mean-equator-of-date vector is used as TEME (the frames differ by the nutation in
// right ascension, under 0.005 degrees).
//
// Shadow: conical umbra and penumbra of a spherical Earth (radius 6378.137 km) lit by a spherical Sun (696,000 km).  With s the
// unit vector to the Sun, x = -r.s the distance behind the Earth's centre along the shadow axis and h = |r x s| the distance
// from the axis (= sqrt(|r|^2 - x^2), in the form that does not cancel near the axis),
//     f_umbra    = h - (R - x tan a_u),  sin a_u = (R_sun - R) / d
//     f_penumbra = h - (R + x tan a_p),  sin a_p = (R_sun + R) / d
// and a point is in that shadow when x > 0 and f < 0.  Not modelled: the Earth's oblateness, atmospheric refraction, light time.
#pragma once

#define AZ_AU_KM 149597870.7
#define AZ_SHADOW_R_EARTH 6378.137
#define AZ_SHADOW_R_SUN 696000.0

// the model; sincos(angle rad, sin, cos) is az_sincos on the device and libm on the host
template <class SinCos>
__host__ __device__ inline void az_sun_model(double jd, double s[3], SinCos &&sincos)
{
    const double rad = AZ_PI / 180.0;
    const double T = (jd - 2451545.0) / 36525.0;
    double lm = 280.460 + 36000.771 * T, M = 357.5291092 + 35999.05034 * T;
    lm -= 360.0 * floor(lm / 360.0);
    M -= 360.0 * floor(M / 360.0);
    double s1, c1, s2, c2, sl, cl, se, ce;
    sincos(M * rad, s1, c1);
    sincos(2.0 * (M * rad), s2, c2);
    const double le = lm + 1.914666471 * s1 + 0.019994643 * s2;
    const double r = (1.000140612 - 0.016708617 * c1 - 0.000139589 * c2) * AZ_AU_KM;
    sincos(le * rad, sl, cl);
    sincos((23.439291 - 0.0130042 * T) * rad, se, ce);
    s[0] = r * cl;
    s[1] = r * (ce * sl);
    s[2] = r * (se * sl);
}
__device__ __forceinline__ void az_sun_teme(double jd, double s[3])
{
    az_sun_model(jd, s, [](double a, double &sn, double &cs) { az_sincos(a, sn, cs); });
}

// one grid time's Sun, as the shadow function wants it
struct AzSunPoint {
    double s[3];         // unit vector to the Sun (TEME)
    double d;            // its distance, km
    double tan_u, tan_p; // tangents of the half angles of the umbra and penumbra cones
};
// sun_km -> the record; rsqrt(x) = 1 / sqrt(x)
template <class Rsqrt>
__host__ __device__ inline AzSunPoint az_sun_point(const double sun_km[3], Rsqrt &&rsqrt)
{
    const double d2 = sun_km[0] * sun_km[0] + sun_km[1] * sun_km[1] + sun_km[2] * sun_km[2];
    const double inv = rsqrt(d2);
    AzSunPoint q;
    q.s[0] = sun_km[0] * inv; q.s[1] = sun_km[1] * inv; q.s[2] = sun_km[2] * inv;
    q.d = d2 * inv;
    const double su = (AZ_SHADOW_R_SUN - AZ_SHADOW_R_EARTH) * inv, sp = (AZ_SHADOW_R_SUN + AZ_SHADOW_R_EARTH) * inv;
    q.tan_u = su * rsqrt(1.0 - su * su);
    q.tan_p = sp * rsqrt(1.0 - sp * sp);
    return q;
}

// x, f_umbra and f_penumbra of position r; h^2 is a sum of squares, so the root needs no clamp
struct AzShadow {
    double x, h, fu, fp;
};
template <class Rsqrt>
__host__ __device__ inline AzShadow az_shadow(const double r[3], const AzSunPoint &q, Rsqrt &&rsqrt)
{
    AzShadow o;
    o.x = -(r[0] * q.s[0] + r[1] * q.s[1] + r[2] * q.s[2]);
    const double cx = r[1] * q.s[2] - r[2] * q.s[1], cy = r[2] * q.s[0] - r[0] * q.s[2], cz = r[0] * q.s[1] - r[1] * q.s[0];
    const double h2 = cx * cx + cy * cy + cz * cz;
    o.h = h2 > 0.0 ? h2 * rsqrt(h2) : 0.0;
    o.fu = o.h - (AZ_SHADOW_R_EARTH - o.x * q.tan_u);
    o.fp = o.h - (AZ_SHADOW_R_EARTH + o.x * q.tan_p);
    return o;
}
// 0 sunlit, 1 penumbra only, 2 umbra
__host__ __device__ inline int az_shadow_state(const AzShadow &o)
{
    return o.x > 0.0 ? (o.fu < 0.0 ? 2 : o.fp < 0.0 ? 1 : 0) : 0;
}
