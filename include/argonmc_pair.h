/* argonmc_pair.h — the sampled pair distribution: per region of a spatial grid, a histogram of the distance from every particle
 * of the region to every other particle of the system, and of those pairs that still approach each other (DESIGN.md 17;
 * opt-in).  Included by argonmc.h; the ABI version is argonmc.h's (additions only).
 *
 * The reference has no such output.  A sample looks at the final state of the step, read through the last sweep's deferred
 * results like the sampled fields do:
 *   centre        a particle i of the context's range [lo, hi) whose position lies in a region of the grid by the bin rule of the
 *                 sampled fields in argonmc.h (w = (hi - lo) / n, floor((u - lo) / w), u == hi in the last bin, NaN outside;
 *                 axisymmetric: r = sqrt(x*x + y*y) and z).  A particle of the range outside the grid only adds to n_outside.
 *   neighbour     every particle j != i of the WHOLE system, in a region or not, in the range or not.  Particle indices are
 *                 compared, not positions: coincident particles are a pair with r = 0.
 *   distance      per ordered pair dx = x_i - x_j (dy, dz alike), r2 = (dx*dx + dy*dy) + dz*dz, r = sqrt(r2): IEEE double as
 *                 written, no FMA.  The pair counts iff r < r_max, in the column
 *                   k = floor(r / (r_max / H))      the rule of one axis over [0, r_max] with H = hist_bins
 *                 (a quotient that rounds up to H with r < r_max lands in the last column, as u == hi does).
 *   approaching   s = (dx*dvx + dy*dvy) + dz*dvz with dv = v_i - v_j; the pair approaches iff s < 0 (false for NaN).  r and s are
 *                 bitwise the same for (i, j) and (j, i).
 * Every region has C = 1 + 2 * H columns of plain 64-bit counts, in this order:
 *   centres | pairs[0..H) | approaching[0..H)
 * so an unordered pair adds once to the region of each of its ends that is a centre.
 * The search box is the grid's bounding box ([-hi_r, hi_r]^2 x [lo_z, hi_z] on an axisymmetric grid) grown by r_max on every
 * side, cut into min(floor(extent / (r_max * (1 + 2^-20))), 128) (at least 1) cells per axis by the rule of one axis.  A particle
 * that rule puts in no cell — a NaN coordinate, a position outside the box — is UNFILED: it is neither a centre nor a neighbour
 * (it is further than r_max from every region) and only adds to n_unfiled; n_unfiled counts the particles of the whole system,
 * n_outside those of [lo, hi) that are filed but in no region.
 * Nothing is quantised, so the sampler has no error word: a NaN velocity makes s NaN (not approaching), a NaN position leaves the
 * particle unfiled.  At most 2^24 particles in the system.  Everything is integer: the totals do not depend on launch geometry,
 * on the order within a cell or on how the index range is split over ranks (the ranks' totals and n_outside add up to a single
 * context's; n_unfiled is the same on every rank).
 * Index-range shards (amc_set_shard): in the CUBE every rank holds the final state of every particle at the hook, and a rank
 * counts the centres of its own range against everybody.  In the PORE geometries a shard's step ends with the owner's bounds
 * pass, after which the other shards' final state is not resident on this rank: there amc_pair_config, amc_pair_sample and the
 * cadence hook (amc_mg_finish) fail with AMC_ERR_STATE on a context whose range is not the whole system.
 * Samples come from the cadence (`every`: the hooks of the sampled fields, a sample sees the step's final state) or from
 * amc_pair_sample.  The sampler is self-contained.  amc_reset_outputs leaves it alone.  Without a grid every call but
 * amc_pair_config returns AMC_ERR_STATE, and nothing is allocated or launched. */
#ifndef ARGONMC_PAIR_H
#define ARGONMC_PAIR_H
#define AMC_PAIR_MAX_HIST_BINS 256
#define AMC_PAIR_MAX_COLUMNS 6144   /* n1 * n2 * n3 * (1 + 2 * hist_bins): one workgroup's table of 64-bit counters, 48 KiB of LDS */
#define AMC_PAIR_MAX_CELLS_AXIS 128 /* cells of the search box per axis                                                          */
typedef struct amc_pair_grid {
    int32_t struct_size;          /* sizeof(amc_pair_grid)                                                        */
    int32_t kind;                 /* AMC_FIELDS_CARTESIAN | AMC_FIELDS_AXISYMMETRIC (n3 == 1, lo[0] == 0)         */
    int32_t n1, n2, n3;           /* regions per axis; n1 * n2 * n3 * (1 + 2 * hist_bins) <= AMC_PAIR_MAX_COLUMNS */
    int32_t hist_bins;            /* 1 .. AMC_PAIR_MAX_HIST_BINS columns over [0, r_max)                          */
    int64_t every;                /* > 0: a sample after every completed step whose step counter + step_offset is a
                                     multiple of `every`; 0: amc_pair_sample only                                 */
    int64_t step_offset;          /* >= 0, as in amc_field_grid                                                   */
    double lo[3], hi[3];          /* as in amc_field_grid                                                         */
    double r_max;                 /* finite, > 0: pairs closer than this are counted                              */
    int64_t reserved[2];          /* 0                                                                            */
} amc_pair_grid;
/* NULL disables sampling and frees its memory.  A (new) grid starts from zero totals. */
int amc_pair_config(amc_ctx *ctx, const amc_pair_grid *grid);
/* one sample of the current state, enqueued on the context's stream (no synchronisation) */
int amc_pair_sample(amc_ctx *ctx);
/* totals[regions][1 + 2 * hist_bins], samples taken, particles of the range outside the grid, particles of the system unfiled;
 * any may be NULL; synchronises */
int amc_pair_read(amc_ctx *ctx, int64_t *totals, int64_t *n_samples, int64_t *n_outside, int64_t *n_unfiled);
/* the inverse of amc_pair_read (checkpoints) */
int amc_pair_load(amc_ctx *ctx, const int64_t *totals, int64_t n_samples, int64_t n_outside, int64_t n_unfiled);
/* zero totals and counters */
int amc_pair_reset(amc_ctx *ctx);
#endif /* ARGONMC_PAIR_H */
