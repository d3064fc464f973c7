// amc_sample_dev.h — what the samplers of the particle state share on the device (amc_fields.hip, amc_corr.hip): the bin grid as
// the kernels take it, the bin rule of one axis and the read of a particle's final state through the deferred
// results of the last sweep.
#pragma once
#include "amc_internal.h"

struct amc_fields_grid_dev {
    int kind, n1, n2, n3, bins;
    double lo[3], hi[3], w[3];
};

// bin of one coordinate: -1 outside (below lo, at or beyond n bins, NaN); u == hi lands in the last bin
AMC_DEV int amc_fields_axis(double u, double lo, double hi, double w, int n)
{
    const double f = floor((u - lo) / w);
    if (!(f >= 0.0)) return -1;
    if (f >= (double)n) return (f == (double)n && u <= hi) ? n - 1 : -1;
    return (int)f;
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
