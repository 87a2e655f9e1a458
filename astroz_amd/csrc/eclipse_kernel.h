// eclipse_kernel.h -- Earth-shadow intervals over a TEME scratch array (azh_find_eclipses_*).  Included only by astroz_hip.hip,
// after passes_kernel.h (az_herm_root) and sun.h.
//
// Input: one row window of AZ_OUT_TEME output with velocities, satellite-major -- per row and grid point the position, the
// velocity and the propagation error code -- and the call's Sun table, one AzSunPoint per grid time.  Same mapping as k_passes:
// one wave per row, lanes on 64 consecutive grid points, every load a coalesced run of the row (the Sun table is the same
// n_times x 48 bytes for every row: it stays in L2).  A point is "in" when it propagated (err == 0), lies behind the Earth
// (x > 0) and f < 0 for the kind asked for; entries and exits are the 0 -> 1 and 1 -> 0 transitions of the 64-bit ballot of that
// predicate with the last lane's state carried.  The lane that owns an event refines it alone, all event lanes of a chunk at
// once; the wave then walks the event bits in lane order with the interval under way in wave-uniform registers.  There is
// nothing like a culmination to find, so an interval costs two refinements and one 32-byte store.
//
// Refinement (nothing is propagated again): on the bracketing interval [t0, t1] the event time is the root of the cubic
// Hermite interpolant of g = max(f, -x) -- values and 60 dt dg/dt at both ends.  g has the sign of the predicate everywhere
// (g < 0 <=> x > 0 and f < 0), which f alone has not: f is also negative in the mirror cone on the day side.  Wherever a
// satellite can cross the shadow boundary g is f; the -x branch only keeps the root finder's bracket honest on grids so coarse
// that a row goes from the day-side cone into the shadow within one step.  The rate of f follows from r, v and the rate of the
// Sun direction, which is the table's difference quotient over the interval (1 degree a day: 1.4e-3 km/s at LEO radius, against
// 7 km/s of the satellite -- left out it would move an event by about a millisecond).  Open ends (grid start / end, a failed
// neighbour) keep the grid time.
#pragma once
#include "../../include/astroz_hip.h"

struct EclipseArgs {
    const double *pos, *vel;  // [row - row0][n_times][3]: TEME position km, velocity km/s
    const unsigned char *err; // [row - row0][n_times]
    const double *times;      // the caller's time axis (minutes), strictly increasing
    const AzSunPoint *sun;    // [n_times]
    unsigned n_times;
    unsigned row0, n_rows; // catalog rows [row0, row0 + n_rows) of this window
    int penumbra;          // kind: 0 umbra, 1 any shadow
    azh_eclipse *out;      // [n_sats][max_eclipses]
    unsigned max_eclipses;
    uint32_t *n_eclipses; // [n_sats]
    unsigned char *state; // [n_sats][n_times] or null: 0 sunlit, 1 penumbra, 2 umbra, 255 failed
};

// the call's Sun table: jd = reference_jd + times / 1440
__global__ void __launch_bounds__(64) k_sun_table(const double *times, unsigned n, double reference_jd, AzSunPoint *out)
{
    const unsigned i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    double s[3];
    az_sun_teme(reference_jd + times[i] / 1440.0, s);
    out[i] = az_sun_point(s, [](double x) { return az_rsqrt(x); });
}
// device known answers of az_sun_teme (azh_selftest_sun)
__global__ void __launch_bounds__(64) k_sun_kat(const double *jd, unsigned n, double *out3n)
{
    const unsigned i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    double s[3];
    az_sun_teme(jd[i], s);
    out3n[3 * (size_t)i] = s[0]; out3n[3 * (size_t)i + 1] = s[1]; out3n[3 * (size_t)i + 2] = s[2];
}

// g = max(f, -x) and 60 dt dg/dt at one end of an interval; sd = the Sun direction's rate (per second) over the interval
__device__ __forceinline__ void az_shadow_g(const double *r, const double *v, const AzSunPoint &q, const double sd[3], int penumbra,
                                            double k, double &g, double &m)
{
    const AzShadow o = az_shadow(r, q, [](double x) { return az_rsqrt(x); });
    const double xd = -(v[0] * q.s[0] + v[1] * q.s[1] + v[2] * q.s[2]) - (r[0] * sd[0] + r[1] * sd[1] + r[2] * sd[2]);
    const double rv = r[0] * v[0] + r[1] * v[1] + r[2] * v[2];
    const double hd = o.h > 0.0 ? (rv - o.x * xd) * az_rcp(o.h) : 0.0; // h^2 = |r|^2 - x^2
    const double f = penumbra ? o.fp : o.fu, fd = penumbra ? hd - xd * q.tan_p : hd + xd * q.tan_u;
    const bool cone = f >= -o.x;
    g = cone ? f : -o.x;
    m = k * (cone ? fd : -xd);
}

#define AZ_ECLIPSE_WAVES 4
__global__ void __launch_bounds__(64 * AZ_ECLIPSE_WAVES) k_eclipses(EclipseArgs p)
{
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wrow = blockIdx.x * AZ_ECLIPSE_WAVES + (threadIdx.x >> 6);
    if (wrow >= p.n_rows) return; // (wave-uniform)
    const unsigned n = p.n_times;
    const size_t srow = (size_t)p.row0 + wrow;
    const double *P = p.pos + (size_t)wrow * n * 3, *V = p.vel + (size_t)wrow * n * 3;
    const unsigned char *E = p.err + (size_t)wrow * n;
    const double *T = p.times;
    azh_eclipse *out = p.out + srow * p.max_eclipses;
    unsigned char *S = p.state ? p.state + srow * n : nullptr;

    azh_eclipse cur{}; // the interval under way (wave-uniform)
    unsigned count = 0;
    bool in_shadow = false;
    uint64_t carry_bad = 0; // the grid point before this iteration's first failed
    for (unsigned base = 0; base < n; base += 64) {
        const unsigned i = base + lane;
        const bool live = i < n;
        bool bad = false, in = false;
        if (live) {
            const double r[3] = {P[3 * (size_t)i], P[3 * (size_t)i + 1], P[3 * (size_t)i + 2]};
            bad = E[i] != 0;
            const AzShadow o = az_shadow(r, p.sun[i], [](double x) { return az_rsqrt(x); });
            const int st = az_shadow_state(o);
            in = !bad && (p.penumbra ? st >= 1 : st == 2);
            if (S) S[i] = bad ? (unsigned char)255 : (unsigned char)st;
        }
        const uint64_t m = __ballot(in), mb = __ballot(bad), ml = __ballot(live);
        const uint64_t prev = (m << 1) | (uint64_t)in_shadow, prevb = (mb << 1) | carry_bad;
        const uint64_t entries = m & ~prev, exits = ~m & prev & ml;
        carry_bad = mb >> 63;
        in_shadow = (m >> (__builtin_popcountll(ml) - 1)) & 1u; // the last live point's state (live lanes are 0 .. k)
        uint64_t ev = entries | exits;
        if (ev == 0) continue;
        // refinement by the lane that owns the event: an entry on [i-1, i] (i first point inside) or an exit on [i-1, i]
        // (i-1 last point inside)
        double ev_t = 0.0;
        unsigned ev_fl = 0;
        if ((ev >> lane) & 1u) {
            const bool is_entry = (entries >> lane) & 1u;
            if (is_entry && i == 0) {
                ev_t = T[0];
                ev_fl = AZH_ECLIPSE_IN_AT_START;
            } else if (is_entry ? (bool)((prevb >> lane) & 1u) : bad) {
                ev_t = T[is_entry ? i : i - 1]; // the open end stays on the grid point that propagated
                ev_fl = AZH_ECLIPSE_CUT_BY_ERROR;
            } else {
                const size_t i0 = i - 1;
                const AzSunPoint q0 = p.sun[i0], q1 = p.sun[i];
                const double dt = T[i] - T[i0], k = 60.0 * dt, ik = az_rcp(k);
                const double sd[3] = {(q1.s[0] - q0.s[0]) * ik, (q1.s[1] - q0.s[1]) * ik, (q1.s[2] - q0.s[2]) * ik};
                double g0, m0, g1, m1;
                az_shadow_g(P + 3 * i0, V + 3 * i0, q0, sd, p.penumbra, k, g0, m0);
                az_shadow_g(P + 3 * (size_t)i, V + 3 * (size_t)i, q1, sd, p.penumbra, k, g1, m1);
                ev_t = fma(az_herm_root(g0, g1, m0, m1), dt, T[i0]);
            }
        }
        // the events in lane order: an entry opens a record, an exit closes and stores it
        while (ev) {
            const unsigned L = (unsigned)__builtin_ctzll(ev);
            ev &= ev - 1u;
            const double t_e = az_readlane_f64(ev_t, L);
            const unsigned fl_e = az_readlane_u32(ev_fl, L);
            if ((entries >> L) & 1u) {
                cur.t_entry_min = t_e;
                cur.flags = fl_e;
                cur.grid_entry = base + L;
            } else {
                cur.t_exit_min = t_e;
                cur.flags |= fl_e;
                cur.grid_exit = base + L - 1u;
                if (lane == 0 && count < p.max_eclipses) out[count] = cur;
                ++count;
            }
        }
    }
    if (in_shadow) { // still inside at the last grid point
        cur.t_exit_min = T[n - 1u];
        cur.flags |= AZH_ECLIPSE_IN_AT_END;
        cur.grid_exit = n - 1u;
        if (lane == 0 && count < p.max_eclipses) out[count] = cur;
        ++count;
    }
    if (lane == 0) p.n_eclipses[srow] = count;
}
