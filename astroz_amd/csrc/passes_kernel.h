// passes_kernel.h -- ground-station pass search over a topocentric scratch array (azh_find_passes_*).  Included only by
// astroz_hip.hip, after kernels.h.
//
// Input: one row window of AZ_OUT_TOPOCENTRIC output with rates, satellite-major -- per row and grid point (az, el, range),
// (az rate, el rate, range rate) and the propagation error code.  One wave per row, lanes on 64 consecutive grid points: every
// load is a coalesced run of the row.  A point is "up" when it propagated (err == 0) and el >= min_el; rises and sets are the
// 0 -> 1 and 1 -> 0 transitions of a 64-bit ballot of that predicate, with the last lane's state carried from one iteration to
// the next.  Events are rare (at most ~16 per LEO satellite and day against 1,440 grid points), so the lane that owns an event
// refines it alone and the wave then walks the event bits in lane order, keeping the pass under way in wave-uniform registers;
// the running maximum of a pass is a wave max over the lanes of its segment.
//
// Refinement (nothing is propagated again): on the bracketing interval [t0, t1] of a rise or set, elevation is the cubic
// Hermite interpolant of (el, el rate x 60) at both ends -- per minute, over the true interval length -- and the event time is
// its root inside the bracket: safeguarded Newton from the linear estimate, bisection whenever a step leaves the bracket.  The
// azimuth there is interpolated the same way after unwrapping a1 to within pi of a0.  The culmination is the grid maximum of
// the pass; on each of its two adjacent intervals where the elevation rate changes sign (+ to -) the highest point of the
// Hermite-interpolated topocentric track (az_culmination) replaces it if it is higher.  Open ends (grid start / end, a failed
// neighbour) keep the grid value.
#pragma once
#include "../../include/astroz_hip.h"

struct PassArgs {
    const double *pos, *vel;  // [row - row0][n_times][3]: (az, el, range), (az rate, el rate, range rate)
    const unsigned char *err; // [row - row0][n_times]
    const double *times;      // the caller's time axis (minutes), strictly increasing
    unsigned n_times;
    unsigned row0, n_rows; // catalog rows [row0, row0 + n_rows) of this window
    double min_el;         // rad
    azh_pass *out;         // [n_sats][max_passes]
    unsigned max_passes;
    uint32_t *n_passes; // [n_sats]
};

// cubic Hermite on s in [0, 1]: values f0, f1, end slopes m0, m1 (already scaled by the interval length)
__device__ __forceinline__ double az_herm(double f0, double f1, double m0, double m1, double s)
{
    const double s2 = s * s, s3 = s2 * s;
    return (2.0 * s3 - 3.0 * s2 + 1.0) * f0 + (s3 - 2.0 * s2 + s) * m0 + (3.0 * s2 - 2.0 * s3) * f1 + (s3 - s2) * m1;
}
__device__ __forceinline__ double az_herm_d(double f0, double f1, double m0, double m1, double s)
{
    return (6.0 * s * s - 6.0 * s) * (f0 - f1) + (3.0 * s * s - 4.0 * s + 1.0) * m0 + (3.0 * s * s - 2.0 * s) * m1;
}
// root in [0, 1] of the Hermite interpolant (f0 and f1 of opposite sign or zero): safeguarded Newton from the linear estimate
__device__ __forceinline__ double az_herm_root(double f0, double f1, double m0, double m1)
{
    auto g = [&](double s) { return az_herm(f0, f1, m0, m1, s); };
    auto dg = [&](double s) { return az_herm_d(f0, f1, m0, m1, s); };
    const double g0 = f0, g1 = f1;
    if (g0 == 0.0) return 0.0;
    if (g1 == 0.0) return 1.0;
    double lo = 0.0, hi = 1.0, s = g0 / (g0 - g1);
    for (int it = 0; it < 64; ++it) {
        const double gs = g(s);
        if (gs == 0.0) break;
        if ((gs < 0.0) == (g0 < 0.0)) lo = s;
        else hi = s;
        const double d = dg(s);
        double sn = d != 0.0 ? s - gs / d : lo;
        if (!(sn > lo && sn < hi)) sn = 0.5 * (lo + hi);
        const bool done = fabs(sn - s) <= 1e-15;
        s = sn;
        if (done) break;
    }
    return s;
}
// azimuth on [0, 1]: a1 unwrapped to within pi of a0, Hermite, back into [0, 2 pi)
__device__ __forceinline__ double az_herm_azimuth(double a0, double a1, double m0, double m1, double s)
{
    double d = a1 - a0;
    d -= AZ_TWOPI * rint(d * (1.0 / AZ_TWOPI));
    double a = az_herm(a0, a0 + d, m0, m1, s);
    a -= AZ_TWOPI * floor(a * (1.0 / AZ_TWOPI));
    return (a >= AZ_TWOPI || a < 0.0) ? 0.0 : a;
}

// culmination: the grid points' topocentric ENU positions and velocities (rebuilt from (az, el, range) and their rates) are
// interpolated component by component with cubic Hermites, and the elevation of that track is maximised: the root of the
// sign of its derivative, which the end rates fix, by regula falsi with the Illinois correction (about ten evaluations).
// (Hermite on the elevation itself is good for rises and sets but not at the top of a high pass, whose time scale -- range /
// speed, about a minute in LEO -- is the grid step: 1e-2 rad too low at 60 degrees on a one-minute grid, against 3e-7 rad
// this way; measured on two-body passes.)
__device__ __forceinline__ void az_enu_state(const double *P, const double *V, double c[3][2])
{
    double se, ce, sa, ca;
    az_sincos(P[1], se, ce);
    az_sincos(P[0], sa, ca);
    const double h = P[2] * ce, hd = V[2] * ce - P[2] * se * V[1];
    c[0][0] = h * sa; c[0][1] = hd * sa + h * ca * V[0];        // E, dE/dt
    c[1][0] = h * ca; c[1][1] = hd * ca - h * sa * V[0];        // N
    c[2][0] = P[2] * se; c[2][1] = V[2] * se + P[2] * ce * V[1]; // U
}
// elevation of the highest point of the track on [t0, t1] (dt minutes; the elevation rate is > 0 at t0 and < 0 at t1), and
// its place s in [0, 1]
__device__ __forceinline__ double az_culmination(const double *P0, const double *V0, const double *P1, const double *V1, double dt,
                                                 double &s_out)
{
    double a[3][2], b[3][2];
    az_enu_state(P0, V0, a);
    az_enu_state(P1, V1, b);
    const double k = 60.0 * dt;
    double x[3], xd[3];
    auto track = [&](double s) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            x[j] = az_herm(a[j][0], b[j][0], k * a[j][1], k * b[j][1], s);
            xd[j] = az_herm_d(a[j][0], b[j][0], k * a[j][1], k * b[j][1], s);
        }
    };
    auto slope = [&](double s) { // h^2 r^2 x (d elevation / ds)
        track(s);
        return (x[0] * x[0] + x[1] * x[1]) * xd[2] - x[2] * (x[0] * xd[0] + x[1] * xd[1]);
    };
    double lo = 0.0, hi = 1.0, g_lo = slope(0.0), g_hi = slope(1.0), s = 0.5;
    int side = 0;
    for (int it = 0; it < 40 && g_lo > 0.0 && g_hi < 0.0; ++it) {
        const double sn = (lo * g_hi - hi * g_lo) / (g_hi - g_lo);
        const bool done = fabs(sn - s) <= 1e-14;
        s = sn;
        const double gs = slope(s);
        if (done || gs == 0.0) break;
        if (gs > 0.0) {
            lo = s; g_lo = gs;
            if (side == 1) g_hi *= 0.5;
            side = 1;
        } else {
            hi = s; g_hi = gs;
            if (side == -1) g_lo *= 0.5;
            side = -1;
        }
    }
    s_out = s;
    track(s);
    const double h2 = x[0] * x[0] + x[1] * x[1];
    return az_atan2(x[2], h2 * az_rsqrt(fmax(h2, 1.0e-300)));
}

__device__ __forceinline__ double az_wave_max(double x)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x = fmax(x, __shfl_xor(x, o, 64));
    return x;
}

// ---- the pass tracker both kernels share ---------------------------------------------------------------------------------
// The kernels differ only in where a grid point's look angles come from -- a look functor: look(i, a, ad) fills (az, el, range)
// and their rates at grid point i -- and in where a station's pass state waits between chunks.  The rest is this.
struct AzLookScratch { // the topocentric scratch as it stands
    const double *P, *V;
    __device__ __forceinline__ void operator()(size_t i, double a[3], double ad[3]) const
    {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            a[k] = P[3 * i + k];
            ad[k] = V[3 * i + k];
        }
    }
};
struct AzLookStation { // az_topocentric<true> of the ECEF state of the scratch, from observer o
    AzLookScratch state;
    const AzObserver &o;
    __device__ __forceinline__ void operator()(size_t i, double a[3], double ad[3]) const
    {
        state(i, a, ad);
        az_topocentric<true>(a, ad, o);
    }
};

// one station's pass under way, and what it has stored
struct AzPassState {
    azh_pass cur;
    double best_el;
    unsigned best_i, count;
};
// one row's constants, for one station
struct AzPassRow {
    const unsigned char *E; // the row's error codes
    const double *T;        // the time axis
    azh_pass *out;          // the station's records of the row: max_passes of them
    double min_el;          // rad
    unsigned n, max_passes, lane;
};
__device__ __forceinline__ unsigned az_readlane_u32(unsigned x, unsigned l) { return (unsigned)__builtin_amdgcn_readlane((int)x, (int)l); }

// the record of a pass whose set is known: culmination refinement, store (the first max_passes only)
template <class Look>
__device__ __forceinline__ void az_pass_finish(const AzPassRow &r, const Look &look, AzPassState &u)
{
    double t_c = r.T[u.best_i], e_c = u.best_el;
    const unsigned k = u.best_i;
#pragma unroll
    for (int side = 0; side < 2; ++side) {
        if (side == 0 && k == 0) continue;
        if (side == 1 && k + 1 >= r.n) continue;
        const unsigned i0 = side == 0 ? k - 1 : k, i1 = i0 + 1;
        if (r.E[i0] != 0 || r.E[i1] != 0) continue;
        double a0[3], d0[3], a1[3], d1[3];
        look(i0, a0, d0);
        look(i1, a1, d1);
        if (!(d0[1] > 0.0 && d1[1] < 0.0)) continue;
        const double dt = r.T[i1] - r.T[i0];
        double s;
        const double e = az_culmination(a0, d0, a1, d1, dt, s);
        if (e > e_c) {
            e_c = e;
            t_c = fma(s, dt, r.T[i0]);
        }
    }
    u.cur.t_culm_min = t_c;
    u.cur.max_elevation_rad = e_c;
    u.cur.grid_culm = k;
    if (r.lane == 0 && u.count < r.max_passes) r.out[u.count] = u.cur;
    ++u.count;
}

// one chunk of 64 grid points from base: this lane's elevation el (read only on live lanes) and failure bad, the ballots of up,
// failed (with the point before base in bit 0) and live points.  in_pass (the pass under way, wave-uniform) is the up state of
// the point before base.
template <class Look>
__device__ __forceinline__ void az_pass_chunk(const AzPassRow &r, const Look &look, unsigned base, double el, bool bad, uint64_t m,
                                              uint64_t prevb, uint64_t ml, AzPassState &u, bool &in_pass)
{
    const unsigned lane = r.lane, i = base + lane;
    const bool live = i < r.n;
    const uint64_t prev = (m << 1) | (uint64_t)in_pass;
    const uint64_t rises = m & ~prev, sets = ~m & prev & ml;
    const bool is_rise = (rises >> lane) & 1u, is_set = (sets >> lane) & 1u;
    // refinement by the lane that owns the event: time, azimuth and flag of a rise (interval [i-1, i], i first up point)
    // or a set (interval [i-1, i], i-1 last up point)
    double ev_t = 0.0, ev_az = 0.0;
    unsigned ev_fl = 0;
    if (is_rise || is_set) {
        const bool prev_bad = (prevb >> lane) & 1u;
        if (is_rise && i == 0) {
            double a[3], ad[3];
            look(0, a, ad);
            ev_t = r.T[0];
            ev_az = a[0];
            ev_fl = AZH_PASS_UP_AT_START;
        } else if ((is_rise && prev_bad) || (is_set && bad)) {
            const unsigned j = is_rise ? i : i - 1; // the open end stays on the grid point that propagated
            double a[3], ad[3];
            look(j, a, ad);
            ev_t = r.T[j];
            ev_az = a[0];
            ev_fl = AZH_PASS_CUT_BY_ERROR;
        } else {
            const unsigned i0 = i - 1;
            double a0[3], d0[3], a1[3], d1[3];
            look(i0, a0, d0);
            look(i, a1, d1);
            const double dt = r.T[i] - r.T[i0];
            const double f0 = a0[1] - r.min_el, f1 = a1[1] - r.min_el;
            const double s = az_herm_root(f0, f1, 60.0 * dt * d0[1], 60.0 * dt * d1[1]);
            ev_t = fma(s, dt, r.T[i0]);
            ev_az = az_herm_azimuth(a0[0], a1[0], 60.0 * dt * d0[0], 60.0 * dt * d1[0], s);
        }
    }
    // the segment [lo, hi) of this chunk belongs to the pass under way: its grid maximum (earliest index on ties)
    auto seg_max = [&](unsigned lo, unsigned hi) {
        const bool in = lane >= lo && lane < hi && live;
        const double mx = az_wave_max(in ? el : -1.0e300);
        const uint64_t hit = __ballot(in && el == mx);
        if (hit && mx > u.best_el) {
            u.best_el = mx;
            u.best_i = base + (unsigned)__builtin_ctzll(hit);
        }
    };
    // the events in lane order: a rise opens a record, a set closes it
    uint64_t ev = rises | sets;
    unsigned seg_lo = 0;
    while (ev) {
        const unsigned L = (unsigned)__builtin_ctzll(ev);
        ev &= ev - 1u;
        if (in_pass && L > seg_lo) seg_max(seg_lo, L);
        const double t_e = az_readlane_f64(ev_t, L), az_e = az_readlane_f64(ev_az, L);
        const unsigned fl_e = az_readlane_u32(ev_fl, L);
        if ((rises >> L) & 1u) {
            in_pass = true;
            u.cur = azh_pass{};
            u.cur.t_rise_min = t_e;
            u.cur.rise_azimuth_rad = az_e;
            u.cur.flags = fl_e;
            u.cur.grid_rise = base + L;
            u.best_el = -1.0e300;
            u.best_i = base + L;
        } else {
            u.cur.t_set_min = t_e;
            u.cur.set_azimuth_rad = az_e;
            u.cur.flags |= fl_e;
            u.cur.grid_set = base + L - 1u;
            az_pass_finish(r, look, u);
            in_pass = false;
        }
        seg_lo = L;
    }
    if (in_pass) seg_max(seg_lo, 64u);
}

// a pass still up at the last grid point
template <class Look>
__device__ __forceinline__ void az_pass_close_at_end(const AzPassRow &r, const Look &look, AzPassState &u)
{
    double a[3], ad[3];
    look(r.n - 1, a, ad);
    u.cur.t_set_min = r.T[r.n - 1];
    u.cur.set_azimuth_rad = a[0];
    u.cur.flags |= AZH_PASS_UP_AT_END;
    u.cur.grid_set = r.n - 1;
    az_pass_finish(r, look, u);
}

#define AZ_PASS_WAVES 4
__global__ void __launch_bounds__(64 * AZ_PASS_WAVES) k_passes(PassArgs p)
{
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wrow = blockIdx.x * AZ_PASS_WAVES + (threadIdx.x >> 6);
    if (wrow >= p.n_rows) return; // (wave-uniform)
    const unsigned n = p.n_times;
    const size_t srow = (size_t)p.row0 + wrow;
    const double *P = p.pos + (size_t)wrow * n * 3;
    const unsigned char *E = p.err + (size_t)wrow * n;
    const AzLookScratch look{P, p.vel + (size_t)wrow * n * 3};
    const AzPassRow r{E, p.times, p.out + srow * p.max_passes, p.min_el, n, p.max_passes, lane};

    AzPassState u{}; // the pass under way (wave-uniform)
    u.best_el = -1.0e300;
    bool in_pass = false;
    uint64_t carry_bad = 0; // the grid point before this iteration's first failed
    for (unsigned base = 0; base < n; base += 64) {
        const unsigned i = base + lane;
        const bool live = i < n;
        const double el = live ? P[3 * (size_t)i + 1] : 0.0;
        const bool bad = live && E[i] != 0;
        const bool up = live && !bad && el >= r.min_el;
        const uint64_t m = __ballot(up), mb = __ballot(bad), ml = __ballot(live);
        az_pass_chunk(r, look, base, el, bad, m, (mb << 1) | carry_bad, ml, u, in_pass);
        carry_bad = mb >> 63;
    }
    if (in_pass) az_pass_close_at_end(r, look, u);
    if (lane == 0) p.n_passes[srow] = u.count;
}

// ---- several stations per call (azh_find_passes_stations_*) -------------------------------------------------------------
// Input: one row window of AZ_OUT_ECEF output with velocities, satellite-major -- per row and grid point the Earth-fixed
// position, the rotated velocity and the propagation error code -- and a group of at most 64 stations.  Same mapping as
// k_passes (one wave per row, lanes on 64 consecutive grid points); each chunk's state is loaded once and the stations are
// walked inside the time loop.  Every elevation, azimuth and rate that enters a decision or a record is az_topocentric<true>
// of the stored state, the arithmetic k_rows_fast FRAME 3 applies to the same rotated state, so that a station's records are
// those of k_passes for it.  The up test is first decided without atan2: el >= min_el <=> U |U| >= s |s| |rho|^2
// (s = sin(min_el)); within a relative margin of 1e-12 of |rho|^2 -- far above the rounding of either side -- the exact
// elevation decides.  A chunk with no up lane and no pass under way costs that test only.  The state of station j's pass
// (count, record under way, running maximum) lives in lane j and is read into wave-uniform registers with readlane when the
// station has anything to do in a chunk; whether its pass is under way is bit j of a wave-uniform mask.
struct AzStation {
    AzObserver o;
    double min_el; // rad
    double s2;     // sin(min_el) |sin(min_el)|
};

// The up decision of an Earth-fixed position R seen from station S, the one every kernel that asks "in view?" takes: the
// cheap test above, d = U |U| - s |s| |rho|^2 against a margin of 1e-12 |rho|^2.  Below the margin the position is down and
// el is left alone.  Above it the position is up without more when the caller has no use for the elevation (!WANT_EL);
// otherwise -- inside the margin always -- el is the exact elevation (az_topocentric's) and el >= min_el decides.
template <bool WANT_EL>
__device__ __forceinline__ bool az_station_up(const double R[3], const AzStation &S, double &el)
{
    const double dx = R[0] - S.o.x, dy = R[1] - S.o.y, dz = R[2] - S.o.z;
    const double q = fma(S.o.cos_lon, dx, S.o.sin_lon * dy);
    const double U = fma(S.o.cos_lat, q, S.o.sin_lat * dz);
    const double rho2 = fma(dx, dx, fma(dy, dy, dz * dz));
    const double d = fma(U, fabs(U), -(S.s2 * rho2)), margin = 1.0e-12 * rho2;
    if (!(d >= -margin)) return false;
    if (!WANT_EL && d > margin) return true;
    double a[3] = {R[0], R[1], R[2]}, ad[3] = {0.0, 0.0, 0.0}; // (the position slot does not read the velocity)
    az_topocentric<true>(a, ad, S.o);
    el = a[1];
    return el >= S.min_el;
}

#define AZ_STATION_GROUP 64
struct StationPassArgs {
    const double *pos, *vel;  // [row - row0][n_times][3]: ECEF position, rotated velocity
    const unsigned char *err; // [row - row0][n_times]
    const double *times;      // the caller's time axis (minutes), strictly increasing
    unsigned n_times;
    unsigned row0, n_rows; // catalog rows [row0, row0 + n_rows) of this window
    unsigned n_sats;       // catalog rows in all: the station stride of out / n_passes
    const AzStation *st;   // this group's stations ...
    unsigned n_st, st0;    // ... n_st <= AZ_STATION_GROUP of them, the first being station st0 of the call
    azh_pass *out;         // [n_stations][n_sats][max_passes]
    unsigned max_passes;
    uint32_t *n_passes; // [n_stations][n_sats]
};

// station l's pass state, from lane l into wave-uniform registers
__device__ __forceinline__ AzPassState az_state_of(const AzPassState &s, unsigned l)
{
    AzPassState u;
    u.cur.t_rise_min = az_readlane_f64(s.cur.t_rise_min, l);
    u.cur.t_culm_min = az_readlane_f64(s.cur.t_culm_min, l);
    u.cur.t_set_min = az_readlane_f64(s.cur.t_set_min, l);
    u.cur.max_elevation_rad = az_readlane_f64(s.cur.max_elevation_rad, l);
    u.cur.rise_azimuth_rad = az_readlane_f64(s.cur.rise_azimuth_rad, l);
    u.cur.set_azimuth_rad = az_readlane_f64(s.cur.set_azimuth_rad, l);
    u.cur.flags = az_readlane_u32(s.cur.flags, l);
    u.cur.grid_rise = az_readlane_u32(s.cur.grid_rise, l);
    u.cur.grid_culm = az_readlane_u32(s.cur.grid_culm, l);
    u.cur.grid_set = az_readlane_u32(s.cur.grid_set, l);
    u.best_el = az_readlane_f64(s.best_el, l);
    u.best_i = az_readlane_u32(s.best_i, l);
    u.count = az_readlane_u32(s.count, l);
    return u;
}

__global__ void __launch_bounds__(64 * AZ_PASS_WAVES) k_passes_stations(StationPassArgs p)
{
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wrow = blockIdx.x * AZ_PASS_WAVES + (threadIdx.x >> 6);
    if (wrow >= p.n_rows) return; // (wave-uniform)
    const unsigned n = p.n_times;
    const size_t srow = (size_t)p.row0 + wrow;
    const double *P = p.pos + (size_t)wrow * n * 3, *V = p.vel + (size_t)wrow * n * 3;
    const unsigned char *E = p.err + (size_t)wrow * n;
    auto row = [&](unsigned j, const AzStation &S) { // station j's records of the row, and mask
        return AzPassRow{E, p.times, p.out + ((size_t)(p.st0 + j) * p.n_sats + srow) * p.max_passes, S.min_el, n, p.max_passes, lane};
    };

    AzPassState mine{};      // station `lane`'s
    mine.best_el = -1.0e300;
    uint64_t in_pass_mask = 0; // bit j: station j has a pass under way (its last grid point was up)
    uint64_t carry_bad = 0;    // the grid point before this iteration's first failed

    for (unsigned base = 0; base < n; base += 64) {
        const unsigned i = base + lane;
        const bool live = i < n;
        double R[3] = {0.0, 0.0, 0.0};
        bool bad = false;
        if (live) {
            R[0] = P[3 * (size_t)i];
            R[1] = P[3 * (size_t)i + 1];
            R[2] = P[3 * (size_t)i + 2];
            bad = E[i] != 0;
        }
        const bool ok = live && !bad;
        const uint64_t mb = __ballot(bad), ml = __ballot(live);
        const uint64_t prevb = (mb << 1) | carry_bad;
        for (unsigned j = 0; j < p.n_st; ++j) {
            const AzStation S = p.st[j]; // (wave-uniform)
            bool in_pass = (in_pass_mask >> j) & 1u;
            // (a chunk with nothing up and no pass under way costs the cheap test only; the elevation is read on up lanes only)
            double el = 0.0;
            const uint64_t m = __ballot(ok && az_station_up<true>(R, S, el));
            if (!in_pass && m == 0) continue;

            AzPassState u = az_state_of(mine, j);
            az_pass_chunk(row(j, S), AzLookStation{{P, V}, S.o}, base, el, bad, m, prevb, ml, u, in_pass);
            if (lane == j) mine = u;
            in_pass_mask = in_pass ? (in_pass_mask | (1ull << j)) : (in_pass_mask & ~(1ull << j));
        }
        carry_bad = mb >> 63;
    }
    for (uint64_t open = in_pass_mask; open; open &= open - 1u) {
        const unsigned j = (unsigned)__builtin_ctzll(open);
        const AzStation S = p.st[j];
        AzPassState u = az_state_of(mine, j);
        az_pass_close_at_end(row(j, S), AzLookStation{{P, V}, S.o}, u);
        if (lane == j) mine = u;
    }
    if (lane < p.n_st) p.n_passes[(size_t)(p.st0 + lane) * p.n_sats + srow] = mine.count;
}
