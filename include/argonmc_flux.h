/* argonmc_flux.h — sampled fluxes: the second and third velocity moments per spatial bin, from which the pressure tensor, the
 * energy flux and the heat flux follow (opt-in).  Included by argonmc.h; the ABI version is argonmc.h's
 * (additions only).
 *
 * The reference has no such output.  A sample bins every particle of the context's range [lo, hi) by the rule of the sampled
 * fields in argonmc.h (w = (hi - lo) / n, floor((u - lo) / w), u == hi in the last bin, NaN outside; axisymmetric:
 * r = sqrt(x*x + y*y) and z) and takes the fields' components: (c1, c2, c3) = (vx, vy, vz) on a Cartesian grid; on an
 * axisymmetric grid ((x*vx + y*vy) / r, (x*vy - y*vx) / r, vz) for r > 0 and (vx, vy, vz) on the axis.  Per bin it adds
 * fourteen exact integers, two rows of seven:
 *   row A   count,  q1(c_k) = llrint(c_k * 2^24),  q2(c_k) = llrint((c_k * c_k) * 2^10)   k = 1..3: the fields' seven, bit for bit
 *   row B   0 (reserved, never added to),
 *           llrint((c1 * c2) * 2^10),  llrint((c1 * c3) * 2^10),  llrint((c2 * c3) * 2^10),
 *           q3(c_k) = llrint(ldexp(e * c_k, -6))   k = 1..3,  with e = (c1*c1 + c2*c2) + c3*c3 evaluated in that order
 * (round half to even, IEEE double as written, no FMA).
 * Valid range: |c_k| < 2^14 m/s for every binned particle and at most 2^24 particles per sample.  Then e < 3 * 2^28 and
 * |e * c_k| < 3 * 2^42, so q3 is below 2^38 in magnitude; q1 and q2 are the fields' formats and at most 2^38 (the largest
 * double below 2^14 rounds up to it), so one sample's sums are at most 2^62.  They are added into signed 128-bit totals (low 64 bits, high 64 bits signed).  Everything is integer: the totals do not depend on
 * launch geometry or order.  A binned particle out of range (or NaN) stops the accumulation: its sample adds nothing and no
 * later one does, and amc_flux_read fails with AMC_ERR_CAPACITY naming the lowest such particle index until amc_flux_reset /
 * amc_flux_load / amc_flux_config.  A particle outside the grid only adds to n_outside (its velocity is not examined).
 * Samples come from the cadence (`every`: the hooks of the sampled fields, a sample sees the step's final state) or from
 * amc_flux_sample.  The sampler is self-contained: it does not need the fields switched on.  amc_reset_outputs leaves it
 * alone.  Without a grid every call but amc_flux_config returns AMC_ERR_STATE, and nothing is allocated or launched. */
#ifndef ARGONMC_FLUX_H
#define ARGONMC_FLUX_H
#define AMC_FLUX_MAX_BINS 1024
typedef struct amc_flux_grid {
    int32_t struct_size;          /* sizeof(amc_flux_grid)                                                       */
    int32_t kind;                 /* AMC_FIELDS_CARTESIAN | AMC_FIELDS_AXISYMMETRIC (n3 == 1, lo[0] == 0)        */
    int32_t n1, n2, n3;           /* bins per axis, n1 * n2 * n3 <= AMC_FLUX_MAX_BINS                            */
    int32_t reserved;             /* 0                                                                           */
    int64_t every;                /* > 0: a sample after every completed step whose step counter + step_offset is a
                                     multiple of `every`; 0: amc_flux_sample only                                */
    int64_t step_offset;          /* >= 0, as in amc_field_grid                                                  */
    double lo[3], hi[3];          /* as in amc_field_grid                                                        */
} amc_flux_grid;
/* NULL disables sampling and frees its memory.  A (new) grid starts from zero totals. */
int amc_flux_config(amc_ctx *ctx, const amc_flux_grid *grid);
/* one sample of the current state, enqueued on the context's stream (no synchronisation) */
int amc_flux_sample(amc_ctx *ctx);
/* totals[bins][2][7][2] (rows A, B; seven quantities each; words low, high), samples taken, particles outside; any may be
 * NULL; synchronises */
int amc_flux_read(amc_ctx *ctx, int64_t *totals, int64_t *n_samples, int64_t *n_outside);
/* the inverse of amc_flux_read (checkpoints) */
int amc_flux_load(amc_ctx *ctx, const int64_t *totals, int64_t n_samples, int64_t n_outside);
/* zero totals and counters, clear a pending error */
int amc_flux_reset(amc_ctx *ctx);
#endif /* ARGONMC_FLUX_H */
