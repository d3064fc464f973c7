// amc_sample_dev.h — what the samplers share on the device: the bin rule of one axis (amc_fields.hip, amc_corr.hip;
// amc_surface.hip through amc_surface_bin) and of a position (amc_corr.hip; amc_moments_particle has it written out,
// DESIGN.md 10), the velocity quantisers' range (fields, correlations, fluxes), the carry-add into the 128-bit totals
// (k_sample_reduce, k_surface_accum) and the read of a particle's final state through the deferred results of the last sweep
// (k_moments_accum, k_corr_accum).
#pragma once
#include "amc_internal.h"

#define AMC_SAMPLE_Q 7                  // integers per bin of a table in a slab row (fields: count, q1, q2; correlations: count, m, c; fluxes: two such tables)

// bin of one coordinate: -1 outside (below lo, at or beyond n bins, NaN); u == hi lands in the last bin
AMC_DEV int amc_fields_axis(double u, double lo, double hi, double w, int n)
{
    const double f = floor((u - lo) / w);
    if (!(f >= 0.0)) return -1;
    if (f >= (double)n) return (f == (double)n && u <= hi) ? n - 1 : -1;
    return (int)f;
}

// the linear bin of a position, -1 outside: (x, y, z) on a Cartesian grid, (r, z) on an axisymmetric one
AMC_DEV int amc_sample_bin(const amc_fields_grid_dev &G, double x, double y, double z)
{
    int i1, i2, i3;
    if (G.kind == AMC_FIELDS_CARTESIAN) {
        i1 = amc_fields_axis(x, G.lo[0], G.hi[0], G.w[0], G.n1);
        i2 = amc_fields_axis(y, G.lo[1], G.hi[1], G.w[1], G.n2);
        i3 = amc_fields_axis(z, G.lo[2], G.hi[2], G.w[2], G.n3);
    } else {
        const double r = sqrt(x * x + y * y);
        i1 = amc_fields_axis(r, G.lo[0], G.hi[0], G.w[0], G.n1);
        i2 = amc_fields_axis(z, G.lo[1], G.hi[1], G.w[1], G.n2);
        i3 = 0;
    }
    if (i1 < 0 || i2 < 0 || i3 < 0) return -1;
    return (i1 * G.n2 + i2) * G.n3 + i3;
}

// the velocity quantisers' range: every component below 2^14 m/s in magnitude (false for NaN)
AMC_DEV bool amc_sample_speed_ok(double a, double b, double c) { return fabs(a) < 16384.0 && fabs(b) < 16384.0 && fabs(c) < 16384.0; }

// (lo, hi) += s: a partial sum that wrapped modulo 2^64 (its true value is below 2^63 in magnitude) into a signed 128-bit total
AMC_DEV void amc_add128(unsigned long long &lo, unsigned long long &hi, unsigned long long s)
{
    const unsigned long long now = lo + s;
    hi += (unsigned long long)(((long long)s < 0 ? -1LL : 0LL) + (now < lo ? 1LL : 0LL));
    lo = now;
}

// The state is read through the deferred results of the last sweep (amc_lazy: a particle that collided has its final state
// in the slot arrays until the next streaming pass picks it up) without consuming them: the step sequence is untouched.
AMC_DEV void amc_fields_lazy(const amc_state &S, const amc_lazy &L, long long p, double &x, double &y, double &z, double &vx,
                             double &vy, double &vz)
{
    if (L.enabled) {
        const int sl = L.slot_of[p];
        if (sl >= 0 && L.moved[sl]) {
            const double *t = L.state + (size_t)sl * RS_SLOT_DOUBLES;
            x = t[0]; y = t[1]; z = t[2]; vx = t[3]; vy = t[4]; vz = t[5];
        }
    }
}
