// coverage_kernel.h -- ground coverage over a point grid (azh_coverage_*): per ground point and grid time the number of
// satellites in view, and per point the statistics of that series.  Included only by astroz_hip.hip, after passes_kernel.h
// (AzStation, az_station_up).
//
// Input: one row window of AZ_OUT_ECEF positions, satellite-major, with the propagation error codes (no velocities), and a
// table of AzStation records, one per ground point, padded to a whole number of point blocks with points that see nothing.
// A satellite is in view of a point at a grid time when it propagated there (err == 0) and az_station_up<false> says so: the
// decision k_passes_stations takes, in fp64, with no pre-filter in front of it.
//
// k_coverage_count.  The work is (points x satellites x times) tests of ~15 fp64 operations on a state of 25 bytes, so the
// mapping is chosen for reuse of what is loaded:
//   - lanes sit on 64 consecutive grid times (a chunk): a satellite's chunk is one contiguous run of 1,536 + 64 bytes;
//   - a workgroup of AZ_COV_WAVES waves takes one chunk, AZ_COV_WAVES x AZ_COV_POINTS consecutive points and one slice of the
//     window's rows.  It stages AZ_COV_TILE rows of the chunk in LDS at a time -- a straight copy: lane l reads its position
//     at byte 24 l, and with ds_read_b64 banked on 64 dwords over groups of 32 lanes the stride of 6 dwords is conflict-free
//     (6 l mod 64 takes 32 distinct even values) -- and every wave reads the tile for its own AZ_COV_POINTS points;
//   - a wave holds AZ_COV_SATS satellites' positions in registers and walks its points over them, so that an LDS read is
//     shared by AZ_COV_POINTS tests; the points' constants -- wave-uniform, read from the table with ordinary loads once per
//     slice -- stay in scalar registers (18 each: with 8 points per wave they no longer fit and spill to VGPR lanes), and so
//     do the AZ_COV_POINTS counters of a lane in vector registers.
// Workgroups that share a chunk are neighbours in launch order: the other point blocks' reads of it hit L2.
// Slices exist so that a call with few points still fills the device, hence a (point, time) cell has one writer per slice,
// not per window: the counters are added to `counts` with atomicAdd (no return value; integer sums do not depend on the
// order, so the result is deterministic).  `counts` is zeroed by the caller before the first window.  Every store is a plain
// vector store or vector atomic from C++.
// LDS: AZ_COV_TILE x (1,536 + 64) = 25,600 bytes per workgroup.
//
// k_coverage_stats.  One wave per point scans the point's row of `counts` in chunks of 64 with ballots of
// covered = count >= min_satellites: the run-tracking of k_passes without any refinement.  The gaps (maximal uncovered runs)
// are walked in lane order with the gap under way in wave-uniform registers.
//
// Compile evidence (hipcc --offload-arch=gfx950 -O3, -Rpass-analysis=kernel-resource-usage; neither kernel is a template):
//   k_coverage_count  VGPRs 85, SGPRs 106 (19 spilled to VGPR lanes), scratch 0, LDS 25,600 bytes, occupancy 5 waves per SIMD
//   k_coverage_stats  VGPRs 28, SGPRs 46, scratch 0, LDS 0, occupancy 8
#pragma once
#include "passes_kernel.h"

#define AZ_COV_WAVES 8   // waves of a workgroup: each its own points, all of them one LDS tile
#define AZ_COV_POINTS 4  // points (counters) per lane: their constants stay in scalar registers (18 each) for the whole slice
#define AZ_COV_TILE 16   // rows staged in LDS at a time
#define AZ_COV_SATS 4    // rows held in registers while the points are walked
#define AZ_COV_BLOCK_POINTS (AZ_COV_WAVES * AZ_COV_POINTS)
#define AZ_COV_STAT_WAVES 4 // k_coverage_stats: points (waves) per workgroup

struct CoverageCountArgs {
    const double *pos;        // [row - row0][n_times][3]: ECEF position
    const unsigned char *err; // [row - row0][n_times]
    unsigned n_times;
    unsigned n_rows;     // rows of this window
    unsigned slice_rows; // rows per blockIdx.z: a multiple of AZ_COV_TILE
    const AzStation *pt; // the points, padded to a multiple of AZ_COV_BLOCK_POINTS
    unsigned n_points;   // ... the real ones
    unsigned n_point_blocks; // blockIdx.x = chunk * n_point_blocks + point block: neighbours in launch order share a chunk
    uint32_t *counts;    // [n_points][n_times]
};

__global__ void __launch_bounds__(64 * AZ_COV_WAVES) k_coverage_count(CoverageCountArgs p)
{
    __shared__ double s_pos[AZ_COV_TILE][64 * 3];
    __shared__ unsigned char s_err[AZ_COV_TILE][64];
    const unsigned tid = threadIdx.x, lane = tid & 63u;
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(tid >> 6)); // (wave-uniform, and known to be)
    const unsigned n = p.n_times;
    const unsigned chunk = blockIdx.x / p.n_point_blocks, pblock = blockIdx.x - chunk * p.n_point_blocks;
    const unsigned base = chunk * 64u;                       // first grid time of the chunk
    const unsigned live_t = n - base < 64u ? n - base : 64u; // grid times of the chunk
    const unsigned pt0 = pblock * AZ_COV_BLOCK_POINTS + wave * AZ_COV_POINTS;
    const unsigned row_lo = blockIdx.z * p.slice_rows;
    const unsigned row_hi = p.n_rows - row_lo < p.slice_rows ? p.n_rows : row_lo + p.slice_rows;

    AzStation S[AZ_COV_POINTS]; // (wave-uniform)
    unsigned acc[AZ_COV_POINTS];
#pragma unroll
    for (int j = 0; j < AZ_COV_POINTS; ++j) {
        S[j] = p.pt[pt0 + j];
        acc[j] = 0;
    }

    for (unsigned r0 = row_lo; r0 < row_hi; r0 += AZ_COV_TILE) {
        // stage rows [r0, r0 + AZ_COV_TILE) of the chunk; a row past the window or a time past the grid is marked failed
        __syncthreads(); // (the tile before is read out)
        for (unsigned k = tid; k < AZ_COV_TILE * 192u; k += 64 * AZ_COV_WAVES) {
            const unsigned r = k / 192u, w = k - r * 192u;
            const bool in = r0 + r < row_hi && w < 3u * live_t;
            s_pos[r][w] = in ? p.pos[((size_t)(r0 + r) * n + base) * 3 + w] : 0.0;
        }
        for (unsigned k = tid; k < AZ_COV_TILE * 64u; k += 64 * AZ_COV_WAVES) {
            const unsigned r = k >> 6, w = k & 63u;
            const bool in = r0 + r < row_hi && w < live_t;
            s_err[r][w] = in ? p.err[(size_t)(r0 + r) * n + base + w] : (unsigned char)1;
        }
        __syncthreads();
#pragma unroll 1
        for (unsigned q0 = 0; q0 < AZ_COV_TILE; q0 += AZ_COV_SATS) {
            double R[AZ_COV_SATS][3];
            bool ok[AZ_COV_SATS];
#pragma unroll
            for (int q = 0; q < AZ_COV_SATS; ++q) {
                R[q][0] = s_pos[q0 + q][3 * lane];
                R[q][1] = s_pos[q0 + q][3 * lane + 1];
                R[q][2] = s_pos[q0 + q][3 * lane + 2];
                ok[q] = s_err[q0 + q][lane] == 0;
            }
#pragma unroll
            for (int j = 0; j < AZ_COV_POINTS; ++j) {
#pragma unroll
                for (int q = 0; q < AZ_COV_SATS; ++q) {
                    double el;
                    acc[j] += (ok[q] && az_station_up<false>(R[q], S[j], el)) ? 1u : 0u;
                }
            }
        }
    }
    if (lane < live_t) {
#pragma unroll
        for (int j = 0; j < AZ_COV_POINTS; ++j)
            if (pt0 + j < p.n_points && acc[j] != 0) atomicAdd(p.counts + (size_t)(pt0 + j) * n + base + lane, acc[j]);
    }
}

struct CoverageStatsArgs {
    const uint32_t *counts; // [n_points][n_times]
    const double *times;    // the caller's time axis (minutes), strictly increasing
    unsigned n_times;       // > 0
    unsigned n_points;
    unsigned min_satellites;
    azh_coverage *out; // [n_points]
};

__device__ __forceinline__ unsigned az_wave_min_u32(unsigned x)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x = min(x, (unsigned)__shfl_xor((int)x, o, 64));
    return x;
}
__device__ __forceinline__ unsigned az_wave_max_u32(unsigned x)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x = max(x, (unsigned)__shfl_xor((int)x, o, 64));
    return x;
}
__device__ __forceinline__ unsigned long long az_wave_sum_u64(unsigned long long x)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x += (unsigned long long)__shfl_xor((long long)x, o, 64);
    return x;
}

__global__ void __launch_bounds__(64 * AZ_COV_STAT_WAVES) k_coverage_stats(CoverageStatsArgs p)
{
    const unsigned lane = threadIdx.x & 63u;
    const unsigned pt = blockIdx.x * AZ_COV_STAT_WAVES + (threadIdx.x >> 6);
    if (pt >= p.n_points) return; // (wave-uniform)
    const unsigned n = p.n_times;
    const uint32_t *C = p.counts + (size_t)pt * n;
    const double *T = p.times;

    unsigned lo = 0xffffffffu, hi = 0, n_cov = 0, n_gaps = 0; // lo / hi / sum: this lane's share, reduced at the end
    unsigned long long sum = 0;
    bool in_gap = false; // the grid point before this chunk was uncovered (wave-uniform, like the rest)
    unsigned gap_a = 0;  // ... in the gap that began here
    double best = -1.0;
    unsigned best_a = 0, best_b = 0;
    auto close_gap = [&](unsigned b) { // the gap [gap_a, b]: the longest so far wins, the earliest on ties
        const unsigned i0 = gap_a > 0 ? gap_a - 1 : 0, i1 = b + 1 < n ? b + 1 : n - 1;
        const double len = T[i1] - T[i0];
        if (len > best) {
            best = len;
            best_a = gap_a;
            best_b = b;
        }
    };
    for (unsigned base = 0; base < n; base += 64) {
        const unsigned i = base + lane;
        const bool live = i < n;
        const unsigned c = live ? C[i] : 0u;
        if (live) {
            lo = min(lo, c);
            hi = max(hi, c);
            sum += c;
        }
        const uint64_t ml = __ballot(live);
        const uint64_t cov = __ballot(live && c >= p.min_satellites), unc = ml & ~cov;
        n_cov += (unsigned)__builtin_popcountll(cov);
        const uint64_t prev = (unc << 1) | (uint64_t)in_gap;
        const uint64_t starts = unc & ~prev, ends = cov & prev; // an end at bit L: the gap's last point is L - 1
        for (uint64_t ev = starts | ends; ev; ev &= ev - 1u) {
            const unsigned L = (unsigned)__builtin_ctzll(ev);
            if ((starts >> L) & 1u) {
                gap_a = base + L;
                ++n_gaps;
            } else {
                close_gap(base + L - 1u);
            }
        }
        const unsigned last = (unsigned)__builtin_popcountll(ml) - 1u;
        in_gap = (unc >> last) & 1u;
    }
    if (in_gap) close_gap(n - 1u);
    lo = az_wave_min_u32(lo);
    hi = az_wave_max_u32(hi);
    sum = az_wave_sum_u64(sum);
    if (lane == 0) {
        azh_coverage o{};
        o.mean_in_view = (double)sum / (double)n;
        o.n_covered = n_cov;
        o.min_in_view = lo;
        o.max_in_view = hi;
        o.n_gaps = n_gaps;
        if (n_gaps) {
            o.max_gap_min = best;
            o.grid_gap_start = best_a;
            o.grid_gap_end = best_b;
            o.flags = (best_a == 0 ? AZH_COVERAGE_GAP_AT_START : 0u) | (best_b == n - 1u ? AZH_COVERAGE_GAP_AT_END : 0u);
        }
        p.out[pt] = o;
    }
}
