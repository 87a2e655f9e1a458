// conjunction_kernel.h -- refined close approaches between a fleet of targets and every row of a TEME scratch array
// (azh_find_conjunctions_*).  Included only by astroz_hip.hip, after conjunction.h.
//
// Input: one row window of AZ_OUT_TEME output with velocities, satellite-major -- per row and grid point the position, the
// velocity and the propagation error code -- and the tracks of the targets, laid out the same way (the window itself when it
// holds the whole catalog, else one track per distinct target row in a buffer of the handle; a slot of targets[] names its
// track and its catalog row through two small tables).
//
// The work is (target slots x rows x grid points) tests of 6 subtractions and 3 multiply-adds on a state of 49 bytes per
// object, so the mapping is chosen for reuse of what is loaded:
//   - lanes sit on 64 consecutive grid points and chunks advance by 63, so lane 0 repeats the last point of the chunk before:
//     every grid interval [i - 1, i] has its two ends in lanes l - 1 and l >= 1 of exactly one chunk, and nothing is carried;
//   - a workgroup of AZ_CONJ_WAVES waves takes one chunk, one group of up to AZ_CONJ_GROUP target slots and one slice of the
//     window's rows.  The group's chunk is staged in LDS once, structure-of-arrays by component (s_t[slot][component][point]):
//     lane l reads consecutive doubles, conflict-free ds_read_b64;
//   - each wave walks rows of the slice: it loads its lane's (r, v, err) once per row -- a coalesced run of the row -- takes
//     the left neighbour's r and v from the lane below once per row (__shfl_up), and for every staged slot forms d, w, q.  A
//     bracket needs only the SIGN of q at the two ends and the validity of both, so the neighbour's share is two ballots
//     shifted by one lane: brackets = ok & ok << 1 & neg << 1 & nonneg, no cross-lane move per slot;
//   - rows are sliced (blockIdx.z) until the launch fills the device, as k_coverage_count's are.
// The row data is read once per target group and the target data comes out of LDS.
//
// Refinement is lane-parallel: events need no order inside a row, so there is no wave-serial walk.  A lane notes the slots
// that have a bracket on its interval in a bit mask while the wave runs through the group, and afterwards every lane works
// through its own mask: the prefilter az_ca_far (conjunction.h: chord distance against threshold + the Hermite's largest bend,
// a bound that cannot lose an event), then az_ca_refine, then -- if the miss is below the threshold -- a slot from the
// returning atomicAdd on the one device counter and the record, when the slot is below max_events.  The counter ends as the
// true number of events; which events are kept beyond max_events, and their order, are unspecified.  Every store is a plain
// vector store or vector atomic from C++.
//
// Not events: a slot's own catalog row (skipped by row number), a bracket with a failed point of either object at either end,
// the first and last grid times (no interval to the outside).
// LDS: AZ_CONJ_GROUP x (6 x 512 + 64) + the row table = 50,240 bytes per workgroup.
//
// Compile evidence (hipcc --offload-arch=gfx950 -O3, -Rpass-analysis=kernel-resource-usage):
//   k_conjunctions  VGPRs 104, SGPRs 64, no spills, scratch 0, LDS 50,240 bytes, occupancy 4 waves per SIMD
#pragma once
#include "../../include/astroz_hip.h"
#include "conjunction.h"

#define AZ_CONJ_WAVES 8  // waves of a workgroup: each its own rows, all of them one staged target group
#define AZ_CONJ_GROUP 16 // target slots staged in LDS at a time (the bit mask of a lane's brackets has one bit per slot)
#define AZ_CONJ_STEP 63  // grid points a chunk advances by

struct ConjunctionArgs {
    const double *pos, *vel;   // [row - row0][n_times][3]: TEME position km, velocity km/s
    const unsigned char *err;  // [row - row0][n_times]
    const double *times;       // the caller's time axis (minutes), strictly increasing
    const double *tpos, *tvel; // the targets' tracks: [track][n_times][3]
    const unsigned char *terr; // [track][n_times]
    const unsigned *slot_track; // [n_targets]: the track of a slot ...
    const unsigned *slot_row;   // ... and its catalog row
    unsigned n_times;           // >= 2
    unsigned row0, n_rows;      // catalog rows [row0, row0 + n_rows) of this window
    unsigned slice_rows;        // rows per blockIdx.z
    unsigned n_targets, n_groups; // blockIdx.x = chunk * n_groups + group: neighbours in launch order share a chunk
    double threshold;           // km
    azh_conjunction *out;       // [max_events]
    unsigned max_events;
    uint32_t *n_events; // one counter
};

__global__ void __launch_bounds__(64 * AZ_CONJ_WAVES) k_conjunctions(ConjunctionArgs p)
{
    __shared__ double s_t[AZ_CONJ_GROUP][6][64];
    __shared__ unsigned char s_e[AZ_CONJ_GROUP][64];
    __shared__ unsigned s_row[AZ_CONJ_GROUP];
    const unsigned tid = threadIdx.x, lane = tid & 63u;
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(tid >> 6)); // (wave-uniform, and known to be)
    const unsigned n = p.n_times;
    const unsigned chunk = blockIdx.x / p.n_groups, group = blockIdx.x - chunk * p.n_groups;
    const unsigned base = chunk * AZ_CONJ_STEP;              // first grid point of the chunk (< n - 1)
    const unsigned live_t = n - base < 64u ? n - base : 64u; // grid points of the chunk
    const unsigned slot0 = group * AZ_CONJ_GROUP;
    const unsigned ng = p.n_targets - slot0 < AZ_CONJ_GROUP ? p.n_targets - slot0 : AZ_CONJ_GROUP;
    const unsigned row_lo = blockIdx.z * p.slice_rows;
    const unsigned row_hi = p.n_rows - row_lo < p.slice_rows ? p.n_rows : row_lo + p.slice_rows;

    // stage the group's chunk: [point][3] of the tracks -> [component][point]; a point past the grid is marked failed
    for (unsigned k = tid; k < ng * 384u; k += 64 * AZ_CONJ_WAVES) {
        const unsigned j = k / 384u, rem = k - j * 384u, arr = rem / 192u, w = rem - arr * 192u, l = w / 3u, comp = w - 3u * l;
        const size_t at = ((size_t)p.slot_track[slot0 + j] * n + base) * 3 + w;
        s_t[j][arr * 3u + comp][l] = l < live_t ? (arr ? p.tvel[at] : p.tpos[at]) : 0.0;
    }
    for (unsigned k = tid; k < ng * 64u; k += 64 * AZ_CONJ_WAVES) {
        const unsigned j = k >> 6, l = k & 63u;
        s_e[j][l] = l < live_t ? p.terr[(size_t)p.slot_track[slot0 + j] * n + base + l] : (unsigned char)1;
    }
    if (tid < ng) s_row[tid] = p.slot_row[slot0 + tid];
    __syncthreads();

    const unsigned i = base + lane;
    const bool live = lane < live_t;
    // the interval this lane closes: [i - 1, i] (lanes 1 .. live_t - 1)
    double t_left = 0.0, dt = 1.0;
    if (live && lane > 0) {
        t_left = p.times[i - 1u];
        dt = p.times[i] - t_left;
    }

    for (unsigned r = row_lo + wave; r < row_hi; r += AZ_CONJ_WAVES) { // (wave-uniform)
        const unsigned srow = p.row0 + r;
        double R[3] = {0.0, 0.0, 0.0}, V[3] = {0.0, 0.0, 0.0};
        bool good = false;
        if (live) {
            const size_t at = ((size_t)r * n + i) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                R[c] = p.pos[at + c];
                V[c] = p.vel[at + c];
            }
            good = p.err[(size_t)r * n + i] == 0;
        }
        double RL[3], VL[3]; // the left neighbour's
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            RL[c] = __shfl_up(R[c], 1, 64);
            VL[c] = __shfl_up(V[c], 1, 64);
        }
        unsigned pend = 0; // bit j: slot j of the group has a bracket on this lane's interval
        for (unsigned j = 0; j < ng; ++j) {
            if (s_row[j] == srow) continue; // the target's own row (wave-uniform)
            double d[3], w[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                d[c] = R[c] - s_t[j][c][lane];
                w[c] = V[c] - s_t[j][3 + c][lane];
            }
            const double q = az_ca_dot(d, w);
            const uint64_t ok = __ballot(good && s_e[j][lane] == 0);
            const uint64_t neg = __ballot(q < 0.0), pos = __ballot(q >= 0.0);
            const uint64_t br = ok & (ok << 1) & (neg << 1) & pos;
            pend |= (unsigned)((br >> lane) & 1u) << j;
        }
        while (pend) { // (per lane: its own brackets, in any order)
            const unsigned j = (unsigned)__builtin_ctz(pend);
            pend &= pend - 1u;
            double d0[3], w0[3], d1[3], w1[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                d0[c] = RL[c] - s_t[j][c][lane - 1u];
                w0[c] = VL[c] - s_t[j][3 + c][lane - 1u];
                d1[c] = R[c] - s_t[j][c][lane];
                w1[c] = V[c] - s_t[j][3 + c][lane];
            }
            if (az_ca_far(d0, w0, d1, w1, dt, p.threshold)) continue;
            const AzApproach a = az_ca_refine(d0, w0, d1, w1, dt);
            if (!(a.miss < p.threshold)) continue;
            const unsigned at = atomicAdd(p.n_events, 1u);
            if (at < p.max_events) {
                azh_conjunction o;
                o.t_tca_min = fma(a.sigma, dt, t_left);
                o.miss_km = a.miss;
                o.rel_speed_km_s = a.speed;
                o.target = slot0 + j;
                o.sat = srow;
                o.grid_index = i - 1u;
                o.reserved = 0;
                p.out[at] = o;
            }
        }
    }
}
