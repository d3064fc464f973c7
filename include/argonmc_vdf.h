/* argonmc_vdf.h — sampled velocity distributions: per region of a spatial grid, histograms of the three velocity components
 * and of the speed (opt-in).  Included by argonmc.h; the ABI version is argonmc.h's (additions only).
 *
 * The reference has no such output.  A sample looks at every particle of the context's range [lo, hi), its state read through
 * the last sweep's deferred results like the sampled fields do:
 *   region      the bin rule of the sampled fields in argonmc.h (w = (hi - lo) / n, floor((u - lo) / w), u == hi in the last
 *               bin, NaN outside; axisymmetric: r = sqrt(x*x + y*y) and z).  A particle outside the grid only adds to n_outside
 *               (its velocity is not examined).
 *   components  the fields': (c1, c2, c3) = (vx, vy, vz) on a Cartesian grid; on an axisymmetric grid
 *               ((x*vx + y*vy) / r, (x*vy - y*vx) / r, vz) for r > 0 and (vx, vy, vz) on the axis.
 *   speed       s = sqrt((c1*c1 + c2*c2) + c3*c3), IEEE double as written, no FMA.
 * With H = hist_bins every region has C = 4 * H + 8 columns of plain 64-bit counts, in this order:
 *   count | c1: under, h[0..H), over | c2: under, h[0..H), over | c3: under, h[0..H), over | speed: h[0..H), over
 * and a binned particle adds one to five of them: count; per component the column of
 *   k = floor((c + v_max) / (2 * v_max / H))   the rule of one axis over [-v_max, v_max] (c == v_max in the last bin);
 *                                              no such k: `under` when c < -v_max, else `over`
 * and for the speed the column of
 *   k = floor(s / (v_max / H))                 the rule of one axis over [0, v_max] (s == v_max in the last bin);
 *                                              no such k: `over`.
 * (The quotient is formed from the sum c + v_max, rounded as IEEE double: a component within half an ulp of c + v_max below an
 * edge is counted above it.)  So per region and component under + sum(h) + over == count == sum(h_speed) + over_speed.
 * Valid range: |c_k| < 2^14 m/s for every binned particle, as for the other samplers, and at most 2^24 particles per sample.
 * A binned particle out of range (or NaN) stops the accumulation: its sample adds nothing and no later one does, and
 * amc_vdf_read fails with AMC_ERR_CAPACITY naming the lowest such particle index ("particle <index> ") until amc_vdf_reset /
 * amc_vdf_load / amc_vdf_config.  Everything is integer: the totals do not depend on launch geometry or order.
 * Samples come from the cadence (`every`: the hooks of the sampled fields, a sample sees the step's final state) or from
 * amc_vdf_sample.  The sampler is self-contained.  amc_reset_outputs leaves it alone.  Without a grid every call but
 * amc_vdf_config returns AMC_ERR_STATE, and nothing is allocated or launched. */
#ifndef ARGONMC_VDF_H
#define ARGONMC_VDF_H
#define AMC_VDF_MAX_HIST_BINS 256
#define AMC_VDF_MAX_COLUMNS 24576   /* n1 * n2 * n3 * (4 * hist_bins + 8): one workgroup's table of 32-bit counters, 96 KiB of LDS */
typedef struct amc_vdf_grid {
    int32_t struct_size;          /* sizeof(amc_vdf_grid)                                                        */
    int32_t kind;                 /* AMC_FIELDS_CARTESIAN | AMC_FIELDS_AXISYMMETRIC (n3 == 1, lo[0] == 0)        */
    int32_t n1, n2, n3;           /* regions per axis; n1 * n2 * n3 * (4 * hist_bins + 8) <= AMC_VDF_MAX_COLUMNS */
    int32_t hist_bins;            /* 1 .. AMC_VDF_MAX_HIST_BINS bins of every histogram                          */
    int64_t every;                /* > 0: a sample after every completed step whose step counter + step_offset is a
                                     multiple of `every`; 0: amc_vdf_sample only                                 */
    int64_t step_offset;          /* >= 0, as in amc_field_grid                                                  */
    double lo[3], hi[3];          /* as in amc_field_grid                                                        */
    double v_max;                 /* finite, 0 < v_max <= 16384: components over [-v_max, v_max], speed over [0, v_max] */
    int64_t reserved[2];          /* 0                                                                           */
} amc_vdf_grid;
/* NULL disables sampling and frees its memory.  A (new) grid starts from zero totals. */
int amc_vdf_config(amc_ctx *ctx, const amc_vdf_grid *grid);
/* one sample of the current state, enqueued on the context's stream (no synchronisation) */
int amc_vdf_sample(amc_ctx *ctx);
/* totals[regions][4 * hist_bins + 8], samples taken, particles outside; any may be NULL; synchronises */
int amc_vdf_read(amc_ctx *ctx, int64_t *totals, int64_t *n_samples, int64_t *n_outside);
/* the inverse of amc_vdf_read (checkpoints) */
int amc_vdf_load(amc_ctx *ctx, const int64_t *totals, int64_t n_samples, int64_t n_outside);
/* zero totals and counters, clear a pending error */
int amc_vdf_reset(amc_ctx *ctx);
#endif /* ARGONMC_VDF_H */
