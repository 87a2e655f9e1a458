// TEST-ONLY host emulation of k_rows_fast's tiered loop bodies (fast_step.h AZ_TIER_*), beside emul.cpp.
// One satellite row as the kernel runs it: time segments of `tile` grid points, one window set-up per segment, the body
// tier az_fast_window_tier assigns to the window -- or a FORCED tier -- and lane l producing the points t_lo + l + 64 j.
// The step reports the quantities its window bounds are about through AZ_FAST_PROBE, so that a test can hold the plan's
// bounds against every grid point.  Never built into or loaded by the product.
#define AZ_HOST_EMUL 1
#define AZ_DEVICE static inline
#define AZ_COLD_STRIDE 1
#include <cmath>
#include <cstddef>
#include <cstring>
enum { PROBE_th, PROBE_em, PROBE_eps, PROBE_a_nd, PROBE_NUM };
static double g_probe[PROBE_NUM];
#define AZ_FAST_PROBE(name, value) g_probe[PROBE_##name] = (value);
#include "../../astroz_amd/csrc/init_device.h"
#include "../../astroz_amd/csrc/propagate_device.h"
#include "../../astroz_amd/csrc/fast_step.h"

template <int DELTA, int TIER>
static bool step_as(bool ecc, const FastK& k, const AzGrav& g, double t, FastCarry& st, double r[3], double v[3], double dl)
{
    return ecc ? az_sgp4_fast_step<true, true, DELTA>(k, g, RotCoefLit(), t, st, r, v, dl)
               : az_sgp4_fast_step<true, false, DELTA, TIER>(k, g, RotCoefLit(), t, st, r, v, dl);
}
template <int DELTA>
static bool step_tier(int tier, bool ecc, const FastK& k, const AzGrav& g, double t, FastCarry& st, double r[3], double v[3], double dl)
{
    switch (tier) {
    case AZ_TIER_EPS: return step_as<DELTA, AZ_TIER_EPS>(ecc, k, g, t, st, r, v, dl);
    default: return step_as<DELTA, AZ_TIER_GENERAL>(ecc, k, g, t, st, r, v, dl);
    }
}

extern "C" {

int emul_tiers_num_fields() { return AZ_NUM_FIELDS; }
int emul_tiers_num_probes() { return PROBE_NUM; }
unsigned emul_tiers_init(const double* raw, const double* grav6, double* fields)
{
    AzGrav g{grav6[0], grav6[1], grav6[2], grav6[3], grav6[4], grav6[5], 0.5 * grav6[1]};
    return az_init_satellite(raw, g, fields, 1, 0);
}

// force_tier < 0: every window runs the body of its own tier; >= 0: every accepted window runs that body (only valid
// where force_tier <= the window's tier: the test forces AZ_TIER_GENERAL).  delta (may be null): tight quasi-uniform grid.
// out6: n_times rows (untouched where the window is rejected); tier_out[i]: the tier of point i's window, -1 rejected,
// eccentric form: -1 as well from the first iteration a lane's Newton predicate rejects; probe_out: n_times x PROBE_NUM.
void emul_tiers_row(const double* fields, unsigned flags, const double* grav6, double t_first, double step, int n_times, int tile,
                    int ecc, int force_tier, const float* delta, double dmax, double* out6, int* tier_out, double* probe_out)
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
        const int tier = ecc ? az_fast_window_tier<true>(k, g, w_a, w_b, dmax) : az_fast_window_tier<false>(k, g, w_a, w_b, dmax);
        for (int i = t_lo; i < t_hi; ++i) tier_out[i] = tier;
        if (tier < 0) continue;
        const int body = force_tier >= 0 ? force_tier : tier;
        int first_bad_base = t_hi;
        for (int lane = 0; lane < 64; ++lane) {
            FastCarry st;
            az_seed_fast(fields, 1, 0, fma((double)(t_lo + lane) - 64.0, step, t_first), k.tc_, st);
            for (int base = t_lo; base + lane < t_hi; base += 64) {
                const int i = base + lane;
                double r[3], v[3];
                double t = fma((double)i, step, t_first);
                bool bad;
                if (delta) {
                    const double dl = (double)delta[i];
                    t += dl;
                    bad = step_tier<1>(body, ecc != 0, k, g, t, st, r, v, dl);
                } else {
                    bad = step_tier<0>(body, ecc != 0, k, g, t, st, r, v, 0.0);
                }
                if (bad && base < first_bad_base) first_bad_base = base;
                memcpy(out6 + 6 * (size_t)i, r, 24); memcpy(out6 + 6 * (size_t)i + 3, v, 24);
                for (int q = 0; q < PROBE_NUM; ++q) probe_out[(size_t)i * PROBE_NUM + q] = g_probe[q];
            }
        }
        for (int i = t_lo; i < t_hi; ++i)
            if (t_lo + (i - t_lo) / 64 * 64 >= first_bad_base) tier_out[i] = -1;
    }
}
}
