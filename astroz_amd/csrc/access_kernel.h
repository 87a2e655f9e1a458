// access_kernel.h -- line-of-sight access windows between one target and every row of a TEME scratch array
// (azh_find_access_*).  Included only by astroz_hip.hip, after passes_kernel.h (az_herm_root, the lane readers) and los.h.
//
// Input: one row window of AZ_OUT_TEME output with velocities, satellite-major -- per row and grid point the position, the
// velocity and the propagation error code -- and the target's track, n_times positions, velocities and (for a member of the
// catalog) error codes.  Same mapping as k_eclipses: one wave per row, lanes on 64 consecutive grid points, every load a
// coalesced run of the row (the track is the same n_times x 48 bytes for every row: it stays in L2).  A point has access when
// both objects propagated there (a non-finite track point counts as failed) and g >= 0 (los.h); starts and ends are the
// 0 -> 1 and 1 -> 0 transitions of the 64-bit ballot of that predicate with the last lane's state carried.  The lane that owns
// an event refines it alone, all event lanes of a chunk at once; the wave then walks the event bits in lane order with the
// window under way in wave-uniform registers.  The smallest range of a window is a segmented wave minimum over the lanes of
// its stretch of the chunk, carried across chunks (k_passes's running maximum): a grid value, the earliest index among equal
// minima -- the fused screen's rule -- and not refined.
//
// Refinement (nothing is propagated again): on the bracketing interval [t0, t1] the event time is the root of the cubic
// Hermite interpolant -- values and 60 dt d/dt at both ends -- of the margin that changes sign there: the clearance margin,
// or with a range limit the range margin; when both do, the later root at a start and the earlier at an end, which is where
// their minimum g crosses zero.  (g itself has a kink where the margins cross, and 5,000 km is about the longest line two
// low satellites can have above 100 km: one Hermite through values of g taken from different margins at the two ends was
// measured up to 9 s off there, against 0.01 s for either margin alone.)  Open ends (grid start / end, a failed neighbour of
// either object) keep the grid time.
#pragma once
#include "../../include/astroz_hip.h"

struct AccessArgs {
    const double *pos, *vel;   // [row - row0][n_times][3]: TEME position km, velocity km/s
    const unsigned char *err;  // [row - row0][n_times]
    const double *times;       // the caller's time axis (minutes), strictly increasing
    const double *tpos, *tvel; // the target's track: [n_times][3] each
    const unsigned char *terr; // [n_times] or null (an external track: only non-finite points fail)
    unsigned n_times;
    unsigned row0, n_rows; // catalog rows [row0, row0 + n_rows) of this window
    unsigned skip_row;     // the catalog row that reports nothing (the target itself), or 0xffffffff
    double r_graze;        // Earth radius + grazing altitude, km
    double max_range;      // km; +infinity: no limit
    azh_access *out;       // [n_sats][max_windows]
    unsigned max_windows;
    uint32_t *n_windows;  // [n_sats]
    unsigned char *state; // [n_sats][n_times] or null: 0 Earth in the way, 1 clear but beyond max_range, 2 access, 255 failed
};

__device__ __forceinline__ double az_wave_min(double x)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x = fmin(x, __shfl_xor(x, o, 64));
    return x;
}
__device__ __forceinline__ bool az_finite3(const double *a) { return isfinite(a[0]) && isfinite(a[1]) && isfinite(a[2]); }

#define AZ_ACCESS_WAVES 4
__global__ void __launch_bounds__(64 * AZ_ACCESS_WAVES) k_access(AccessArgs p)
{
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wrow = blockIdx.x * AZ_ACCESS_WAVES + (threadIdx.x >> 6);
    if (wrow >= p.n_rows) return; // (wave-uniform)
    const unsigned n = p.n_times;
    const size_t srow = (size_t)p.row0 + wrow;
    const double *P = p.pos + (size_t)wrow * n * 3, *V = p.vel + (size_t)wrow * n * 3;
    const unsigned char *E = p.err + (size_t)wrow * n;
    const double *T = p.times;
    azh_access *out = p.out + srow * p.max_windows;
    unsigned char *S = p.state ? p.state + srow * n : nullptr;
    auto rsq = [](double x) { return az_rsqrt(x); };

    if (srow == p.skip_row) { // the target's own row: no windows, a state row of 0
        if (S)
            for (unsigned i = lane; i < n; i += 64) S[i] = 0;
        if (lane == 0) p.n_windows[srow] = 0;
        return;
    }

    azh_access cur{}; // the window under way (wave-uniform)
    unsigned count = 0;
    bool in_win = false;
    uint64_t carry_bad = 0; // the grid point before this iteration's first failed
    for (unsigned base = 0; base < n; base += 64) {
        const unsigned i = base + lane;
        const bool live = i < n;
        bool bad = false, in = false;
        double range = 0.0;
        if (live) {
            const double *r1 = P + 3 * (size_t)i, *r2 = p.tpos + 3 * (size_t)i;
            const double a[3] = {r1[0], r1[1], r1[2]}, b[3] = {r2[0], r2[1], r2[2]};
            bad = E[i] != 0 || (p.terr && p.terr[i] != 0) || !az_finite3(b) || !az_finite3(p.tvel + 3 * (size_t)i);
            const AzLos o = az_los(a, b, rsq);
            range = o.range;
            const bool clear = o.clearance - p.r_graze >= 0.0, near = p.max_range - o.range >= 0.0;
            in = !bad && clear && near;
            if (S) S[i] = bad ? (unsigned char)255 : (unsigned char)(clear ? (near ? 2 : 1) : 0);
        }
        const uint64_t m = __ballot(in), mb = __ballot(bad), ml = __ballot(live);
        const uint64_t prev = (m << 1) | (uint64_t)in_win, prevb = (mb << 1) | carry_bad;
        const uint64_t starts = m & ~prev, ends = ~m & prev & ml;
        const bool was_in = in_win;
        carry_bad = mb >> 63;
        in_win = (m >> (__builtin_popcountll(ml) - 1)) & 1u; // the last live point's state (live lanes are 0 .. k)
        uint64_t ev = starts | ends;
        if (ev == 0 && !was_in) continue;
        // refinement by the lane that owns the event: a start on [i-1, i] (i first point with access) or an end on [i-1, i]
        // (i-1 last point with access)
        double ev_t = 0.0;
        unsigned ev_fl = 0;
        if ((ev >> lane) & 1u) {
            const bool is_start = (starts >> lane) & 1u;
            if (is_start && i == 0) {
                ev_t = T[0];
                ev_fl = AZH_ACCESS_OPEN_AT_START;
            } else if (is_start ? (bool)((prevb >> lane) & 1u) : bad) {
                ev_t = T[is_start ? i : i - 1]; // the open end stays on the grid point that propagated
                ev_fl = AZH_ACCESS_CUT_BY_ERROR;
            } else {
                const size_t i0 = i - 1;
                const double dt = T[i] - T[i0], k = 60.0 * dt;
                const AzLosMargins a = az_los_margins(P + 3 * i0, V + 3 * i0, p.tpos + 3 * i0, p.tvel + 3 * i0, p.r_graze, p.max_range, rsq);
                const AzLosMargins b = az_los_margins(P + 3 * (size_t)i, V + 3 * (size_t)i, p.tpos + 3 * (size_t)i, p.tvel + 3 * (size_t)i,
                                                      p.r_graze, p.max_range, rsq);
                const bool by_c = (a.gc < 0.0) != (b.gc < 0.0), by_r = (a.gr < 0.0) != (b.gr < 0.0);
                double s = is_start ? 0.0 : 1.0;
                if (by_c) s = az_herm_root(a.gc, b.gc, k * a.gcd, k * b.gcd);
                if (by_r) {
                    const double sr = az_herm_root(a.gr, b.gr, k * a.grd, k * b.grd);
                    s = !by_c ? sr : is_start ? fmax(s, sr) : fmin(s, sr);
                }
                ev_t = fma(s, dt, T[i0]);
            }
        }
        // lanes [lo, hi) of this chunk belong to the window under way: its smallest range (earliest index on ties)
        auto seg_min = [&](unsigned lo, unsigned hi) {
            const bool inseg = lane >= lo && lane < hi && live;
            const double mn = az_wave_min(inseg ? range : 1.0e300);
            const uint64_t hit = __ballot(inseg && range == mn);
            if (hit && mn < cur.min_range_km) {
                cur.min_range_km = mn;
                cur.grid_min_range = base + (unsigned)__builtin_ctzll(hit);
            }
        };
        // the events in lane order: a start opens a record, an end closes and stores it
        bool open = was_in;
        unsigned seg_lo = 0;
        while (ev) {
            const unsigned L = (unsigned)__builtin_ctzll(ev);
            ev &= ev - 1u;
            if (open && L > seg_lo) seg_min(seg_lo, L);
            const double t_e = az_readlane_f64(ev_t, L);
            const unsigned fl_e = az_readlane_u32(ev_fl, L);
            if ((starts >> L) & 1u) {
                open = true;
                cur.t_start_min = t_e;
                cur.flags = fl_e;
                cur.grid_start = base + L;
                cur.min_range_km = 1.0e300;
                cur.grid_min_range = base + L;
            } else {
                open = false;
                cur.t_end_min = t_e;
                cur.flags |= fl_e;
                cur.grid_end = base + L - 1u;
                if (lane == 0 && count < p.max_windows) out[count] = cur;
                ++count;
            }
            seg_lo = L;
        }
        if (open) seg_min(seg_lo, 64u);
    }
    if (in_win) { // still in access at the last grid point
        cur.t_end_min = T[n - 1u];
        cur.flags |= AZH_ACCESS_OPEN_AT_END;
        cur.grid_end = n - 1u;
        if (lane == 0 && count < p.max_windows) out[count] = cur;
        ++count;
    }
    if (lane == 0) p.n_windows[srow] = count;
}
