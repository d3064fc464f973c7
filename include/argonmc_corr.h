/* argonmc_corr.h — sampled correlations: velocity autocorrelation and mean-square displacement per group and lag
 * (opt-in).  Included by argonmc.h; the ABI version is argonmc.h's (additions only).
 *
 * The reference has no such output.  These are two-time quantities: the device keeps x, y, z, vx, vy, vz of every particle of
 * the context's range [lo, hi) at a time ORIGIN (six origin arrays) and, at every later sample of the window, adds per
 * (group, lag) seven exact integers: the count and, for the Cartesian components k = x, y, z,
 *   m_k = llrint(ldexp(D_k * D_k, 74)),  D_k = u_k - u0_k        (squared displacement, resolution 2^-74 m^2)
 *   c_k = llrint((v_k * v0_k) * 2^10)                            (velocity product, resolution 2^-10 m^2/s^2)
 * (round half to even, IEEE double as written, no FMA).  The components are always Cartesian; the grid only chooses the group.
 * Group: the bin of the particle's ORIGIN position in the group grid, by the rule of the sampled fields in argonmc.h (w = (hi - lo) / n,
 * floor((u - lo) / w), u == hi in the last bin, NaN outside; axisymmetric: r = sqrt(x0*x0 + y0*y0) and z0).  It is recomputed
 * from the stored origin at every sample.  A particle whose origin is outside the grid takes no part in that window (its
 * values are then not examined either) and is counted once per origin in n_outside.
 * Window: samples come from the cadence (`every`) or from amc_corr_sample.  The first sample after amc_corr_config or
 * amc_corr_reset is an origin: it stores the origin arrays and adds lag 0 (m_k = 0, c_k from v_k * v_k).  The next samples are
 * lags 1, 2, ... against that origin.  The sample at lag n_lags is also the next origin: one pass adds lag n_lags against the
 * old origin, stores the new origin and adds lag 0.  The window position (the lag of the next sample, 0: an origin) is host
 * state, like the step counter the cadence reads.
 * The displacement is between the stored and the current position, WHATEVER HAPPENED IN BETWEEN: walls, collisions, the bounds
 * check's recapture, an amc_upload or amc_init_synthetic.  None of these restarts a window; a caller who wants a restart calls
 * amc_corr_reset.  amc_reset_outputs leaves the correlations alone.
 * Valid range per participating particle: |D_k| < 2^-18 m (3.81 um), |v_k| < 2^14 m/s, |v0_k| < 2^14 m/s, and at most 2^24
 * particles per sample: every quantised value is then at most 2^38 in magnitude and one sample's sums at most 2^62.  They are added into signed
 * 128-bit totals (low 64 bits, high 64 bits signed).  Everything is integer: the totals do not depend on launch geometry or
 * order.  A particle out of range (or NaN) stops the accumulation: its sample adds nothing and no later one does, and
 * amc_corr_read fails with AMC_ERR_CAPACITY naming the lowest such particle index until amc_corr_reset / amc_corr_load /
 * amc_corr_config.
 * Limits: groups = n1 * n2 * n3 <= AMC_CORR_MAX_GROUPS, groups * (n_lags + 1) <= AMC_CORR_MAX_CELLS.  A context's range is
 * fixed (amc_set_shard) before amc_corr_config.  Without a grid every call but amc_corr_config returns AMC_ERR_STATE, and
 * nothing is allocated or launched. */
#ifndef ARGONMC_CORR_H
#define ARGONMC_CORR_H
#define AMC_CORR_MAX_GROUPS 256
#define AMC_CORR_MAX_CELLS 65536
typedef struct amc_corr_grid {
    int32_t struct_size;          /* sizeof(amc_corr_grid)                                                       */
    int32_t kind;                 /* AMC_FIELDS_CARTESIAN | AMC_FIELDS_AXISYMMETRIC (n3 == 1, lo[0] == 0)        */
    int32_t n1, n2, n3;           /* groups per axis                                                             */
    int32_t n_lags;               /* >= 1: lags 0 .. n_lags per window                                           */
    int64_t every;                /* > 0: a sample after every completed step whose step counter + step_offset is a
                                     multiple of `every` (the hooks of the sampled fields); 0: amc_corr_sample only */
    int64_t step_offset;          /* >= 0, as in amc_field_grid                                                  */
    double lo[3], hi[3];          /* as in amc_field_grid                                                        */
    int64_t reserved[2];          /* 0                                                                           */
} amc_corr_grid;
/* NULL disables sampling and frees its memory.  A (new) grid starts from zero totals; its first sample is an origin. */
int amc_corr_config(amc_ctx *ctx, const amc_corr_grid *grid);
/* one sample of the current state, enqueued on the context's stream (no synchronisation); advances the window */
int amc_corr_sample(amc_ctx *ctx);
/* totals[groups][n_lags + 1][7][2] (quantities count, m_x m_y m_z, c_x c_y c_z; words low, high), origins stored, samples
 * taken, particles outside (once per origin) and the window position (lag of the next sample); any may be NULL; synchronises */
int amc_corr_read(amc_ctx *ctx, int64_t *totals, int64_t *n_origins, int64_t *n_samples, int64_t *n_outside, int64_t *window_pos);
/* the six origin arrays of the context's range, float64[hi - lo] each (checkpoints); zeros before the first origin */
int amc_corr_origin(amc_ctx *ctx, double *x0, double *y0, double *z0, double *vx0, double *vy0, double *vz0);
/* the inverse of amc_corr_read + amc_corr_origin; the origin arrays may be NULL when window_pos == 0 */
int amc_corr_load(amc_ctx *ctx, const int64_t *totals, int64_t n_origins, int64_t n_samples, int64_t n_outside,
                  int64_t window_pos, const double *x0, const double *y0, const double *z0, const double *vx0,
                  const double *vy0, const double *vz0);
/* zero totals and counters, clear a pending error; the next sample is an origin */
int amc_corr_reset(amc_ctx *ctx);
#endif /* ARGONMC_CORR_H */
