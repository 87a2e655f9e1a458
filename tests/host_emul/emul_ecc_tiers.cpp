// TEST-ONLY host emulation of the tiered loop bodies of k_rows_fast's ECCENTRIC form (fast_step.h AZ_ETIER_*), beside
// emul_tiers.cpp.  One eccentric row as the kernel runs it: time segments of `tile` grid points, one window set-up per
// segment, the body az_fast_window_tier<true> assigns to the window -- or the general body, forced -- and lane l producing
// the points t_lo + l + 64 j.  The step reports what its bounds are about through AZ_FAST_PROBE / AZ_FAST_PROBE_KEPLER.
// Never built into or loaded by the product.
#define AZ_HOST_EMUL 1
#define AZ_DEVICE static inline
#define AZ_COLD_STRIDE 1
#include <cmath>
#include <cstddef>
#include <cstring>
enum { PROBE_th, PROBE_em, PROBE_eps, PROBE_a_nd, PROBE_el2, PROBE_d0, PROBE_d1, PROBE_d2, PROBE_NUM };
static double g_probe[PROBE_NUM];
#define AZ_FAST_PROBE(name, value) g_probe[PROBE_##name] = (value);
#define AZ_FAST_PROBE_KEPLER(name, value) g_probe[PROBE_##name] = (value);
#include "../../astroz_amd/csrc/init_device.h"
#include "../../astroz_amd/csrc/propagate_device.h"
#include "../../astroz_amd/csrc/fast_step.h"

template <int DELTA>
static bool step_tier(int tier, const FastK& k, const AzGrav& g, double t, FastCarry& st, double r[3], double v[3], double dl)
{
    switch (tier) {
    case AZ_ETIER_E1: return az_sgp4_fast_step<true, true, DELTA, AZ_ETIER_E1>(k, g, RotCoefLit(), t, st, r, v, dl);
    case AZ_ETIER_E2: return az_sgp4_fast_step<true, true, DELTA, AZ_ETIER_E2>(k, g, RotCoefLit(), t, st, r, v, dl);
    default: return az_sgp4_fast_step<true, true, DELTA, AZ_TIER_GENERAL>(k, g, RotCoefLit(), t, st, r, v, dl);
    }
}

extern "C" {

int emul_ecc_num_fields() { return AZ_NUM_FIELDS; }
int emul_ecc_num_probes() { return PROBE_NUM; }
unsigned emul_ecc_init(const double* raw, const double* grav6, double* fields)
{
    AzGrav g{grav6[0], grav6[1], grav6[2], grav6[3], grav6[4], grav6[5], 0.5 * grav6[1]};
    return az_init_satellite(raw, g, fields, 1, 0);
}

// the plan's verdict on one window [t_lo, t_hi) of a row of either form: the body tier, -1 rejected (k_plan_windows)
int emul_ecc_plan_tier(const double* fields, unsigned flags, const double* grav6, double t_first, double step, int t_lo, int t_hi, int ecc,
                       double dmax)
{
    AzGrav g{grav6[0], grav6[1], grav6[2], grav6[3], grav6[4], grav6[5], 0.5 * grav6[1]};
    double inc[2 * AZ_INC_NUM];
    const double rate[2] = {fields[F_mdot], fields[F_argpdot]};
    for (int which = 0; which < 2; ++which)
        for (int a = 0; a < 2; ++a)
            az_sincos(rate[a] * (which == 0 ? 64.0 * step : step), inc[AZ_INC_NUM * which + 2 * a], inc[AZ_INC_NUM * which + 2 * a + 1]);
    FastK k;
    az_load_fast(fields, 1, 0, flags, inc, 0, k);
    const double w_a = fma((double)t_lo, step, t_first), w_b = fma((double)(t_hi - 1), step, t_first);
    az_fast_window(fields, 1, 0, w_a, w_b, 64.0 * step, k);
    return ecc ? az_fast_window_tier<true>(k, g, w_a, w_b, dmax) : az_fast_window_tier<false>(k, g, w_a, w_b, dmax);
}

// force_general = 0: every accepted window runs the body of its own tier; 1: the general body (what every window ran before
// the tiers).  delta (may be null): tight quasi-uniform grid.  out6: n_times rows (untouched where the window is rejected);
// tier_out[i]: the tier of point i's window (AZ_TIER_GENERAL, AZ_ETIER_*), -1 rejected; bad_out[i]: the step's Newton
// predicate at point i (the kernel hands the rest of the segment over from the first iteration where a lane raises it);
// probe_out: n_times x PROBE_NUM.
void emul_ecc_row(const double* fields, unsigned flags, const double* grav6, double t_first, double step, int n_times, int tile,
                  int force_general, const float* delta, double dmax, double* out6, int* tier_out, unsigned char* bad_out,
                  double* probe_out)
{
    AzGrav g{grav6[0], grav6[1], grav6[2], grav6[3], grav6[4], grav6[5], 0.5 * grav6[1]};
    double inc[2 * AZ_INC_NUM];
    const double rate[2] = {fields[F_mdot], fields[F_argpdot]};
    for (int which = 0; which < 2; ++which)
        for (int a = 0; a < 2; ++a)
            az_sincos(rate[a] * (which == 0 ? 64.0 * step : step), inc[AZ_INC_NUM * which + 2 * a], inc[AZ_INC_NUM * which + 2 * a + 1]);
    for (int t_lo = 0; t_lo < n_times; t_lo += tile) {
        const int t_hi = t_lo + tile < n_times ? t_lo + tile : n_times;
        FastK k;
        az_load_fast(fields, 1, 0, flags, inc, 0, k);
        const double w_a = fma((double)t_lo, step, t_first), w_b = fma((double)(t_hi - 1), step, t_first);
        az_fast_window(fields, 1, 0, w_a, w_b, 64.0 * step, k);
        const int tier = az_fast_window_tier<true>(k, g, w_a, w_b, dmax);
        for (int i = t_lo; i < t_hi; ++i) tier_out[i] = tier;
        if (tier < 0) continue;
        const int body = force_general ? (int)AZ_TIER_GENERAL : tier;
        for (int lane = 0; lane < 64; ++lane) {
            FastCarry st;
            az_seed_fast(fields, 1, 0, fma((double)(t_lo + lane) - 64.0, step, t_first), k.tc_, st);
            for (int base = t_lo; base + lane < t_hi; base += 64) {
                const int i = base + lane;
                double r[3], v[3];
                double t = fma((double)i, step, t_first);
                for (int q = 0; q < PROBE_NUM; ++q) g_probe[q] = 0.0;
                bool bad;
                if (delta) {
                    const double dl = (double)delta[i];
                    t += dl;
                    bad = step_tier<1>(body, k, g, t, st, r, v, dl);
                } else {
                    bad = step_tier<0>(body, k, g, t, st, r, v, 0.0);
                }
                bad_out[i] = bad ? 1 : 0;
                memcpy(out6 + 6 * (size_t)i, r, 24); memcpy(out6 + 6 * (size_t)i + 3, v, 24);
                for (int q = 0; q < PROBE_NUM; ++q) probe_out[(size_t)i * PROBE_NUM + q] = g_probe[q];
            }
        }
    }
}
}
