/* argonmc_transit.h — sampled transits: entries into, exits from and residence times in zones, with a memory per particle
 * (opt-in).  Included by argonmc.h; the ABI version is argonmc.h's (additions only).
 *
 * The reference has no such output.  A zone is a half-open interval [lo, hi) of one Cartesian coordinate (axis 0, 1, 2: x, y,
 * z); zones may overlap or nest.  A sample looks at every particle of the context's range [lo, hi), its coordinates read
 * through the last sweep's deferred results like the sampled fields do, and compares, per zone, the coordinate u with the
 * bounds as plain IEEE doubles:
 *   below  (1)  u < lo          inside (2)  lo <= u < hi          above  (3)  u >= hi          unknown (0)  never sampled
 * A NaN coordinate on an axis in use stops the accumulation: its sample adds nothing to the totals and no later one does, and
 * amc_transit_read fails with AMC_ERR_CAPACITY naming the lowest such particle index ("particle <index> ") until
 * amc_transit_reset / amc_transit_load / amc_transit_config.
 *
 * Per-particle state, for the particles of the context's range:
 *   state[p]         one 32-bit word, 4 bits per zone (zone k: bits 4k .. 4k+3; zones >= n_zones: 0): bits 0-1 the position
 *                    at the previous sample (0 unknown, 1 below, 2 inside, 3 above); bits 2-3, while the position is inside,
 *                    the side the particle entered from (0 from below, 1 from above, 2 already inside when first seen), else 0
 *   entry[zone][p]   uint32: the index of the sample at which the particle was first seen inside (meaningful while inside)
 *
 * The sample has index s = n_samples before it.  Per particle and zone, previous position a, current position b:
 *   unknown -> inside          entries[2] += 1; entry side 2; entry index s
 *   unknown -> below / above   only the position is stored
 *   below / above -> inside    entries[a == below ? 0 : 1] += 1; that entry side; entry index s
 *   inside -> below / above    an exit of class (entry side e, exit side x = b == below ? 0 : 1) with residence
 *                              tau = s - entry index (>= 1): count += 1, sum_tau += tau, sum_tau2 += tau * tau and one column
 *                              of the histogram, min(floor(log2(tau)), 39)
 *   below -> above, above -> below   skipped += 1: a crossing no sample saw (the cadence is too coarse for the zone)
 * and inside_sum grows by one for every particle inside after the sample.  Then n_samples grows by one.
 *
 * Totals: per zone AMC_TRANSIT_COLUMNS = 263 columns, each a signed 128-bit integer as (low 64 bits, high 64 bits):
 *   0, 1, 2   entries from below, from above, already inside
 *   3         skipped
 *   4         inside_sum
 *   5 + 43 * (2 * e + x) + ...   the exit class (e, x), e = 0, 1, 2 and x = 0, 1:
 *             + 0 count | + 1 sum_tau | + 2 sum_tau2 | + 3 + j, j = 0 .. 39: residences with floor(log2(tau)) == j (j = 39: >= 39)
 * Everything is integer: the totals do not depend on launch geometry or order.
 *
 * Range and exactness: at most 2^24 particles per sample and at most 2^32 - 1 samples since the last reset, load or config.
 * The sample that would be number 2^32 adds nothing and changes no particle's state, nor does any later one, and amc_transit_read
 * fails with AMC_ERR_CAPACITY until reset, load or config.  So tau < 2^32 and tau * tau < 2^64: a launch sums tau (below 2^56),
 * the low and the high 32-bit limb of tau * tau (each below 2^56) as 64-bit integers, and they enter the 128-bit totals with
 * carry — sum_tau and sum_tau2 are exact over the whole range.
 *
 * Tracking sees sampled coordinates and nothing else: amc_upload, amc_init_synthetic and the bounds check's recapture do not
 * restart it (a teleport shows as an entry, an exit or a skipped crossing).  amc_transit_reset and amc_transit_config with a
 * grid zero the totals and n_samples and set every particle to unknown.  amc_reset_outputs leaves the sampler alone.
 * Samples come from the cadence (`every`: the hooks of the sampled fields, a sample sees the step's final state) or from
 * amc_transit_sample.  Without a grid every call but amc_transit_config returns AMC_ERR_STATE, and nothing is allocated or
 * launched. */
#ifndef ARGONMC_TRANSIT_H
#define ARGONMC_TRANSIT_H
#define AMC_TRANSIT_MAX_ZONES 8
#define AMC_TRANSIT_HIST 40             /* histogram columns per exit class                                   */
#define AMC_TRANSIT_CLASS_COLUMNS 43    /* count, sum_tau, sum_tau2, the histogram                            */
#define AMC_TRANSIT_COLUMNS 263         /* 5 + 6 * AMC_TRANSIT_CLASS_COLUMNS                                  */
#define AMC_TRANSIT_MAX_SAMPLES 4294967295LL   /* 2^32 - 1                                                    */
typedef struct amc_transit_grid {
    int32_t struct_size;          /* sizeof(amc_transit_grid)                                                     */
    int32_t n_zones;              /* 1 .. AMC_TRANSIT_MAX_ZONES                                                   */
    int64_t every;                /* > 0: a sample after every completed step whose step counter + step_offset is a
                                     multiple of `every`; 0: amc_transit_sample only                              */
    int64_t step_offset;          /* >= 0, as in amc_field_grid                                                   */
    int32_t axis[AMC_TRANSIT_MAX_ZONES];   /* per zone 0, 1, 2: x, y, z (zones >= n_zones: 0)                     */
    double lo[AMC_TRANSIT_MAX_ZONES];      /* per zone finite lo < hi (zones >= n_zones: 0)                       */
    double hi[AMC_TRANSIT_MAX_ZONES];
    int64_t reserved[2];          /* 0                                                                            */
} amc_transit_grid;
/* NULL disables sampling and frees its memory.  A (new) grid starts from zero totals and every particle unknown. */
int amc_transit_config(amc_ctx *ctx, const amc_transit_grid *grid);
/* one sample of the current state, enqueued on the context's stream (no synchronisation) */
int amc_transit_sample(amc_ctx *ctx);
/* totals[n_zones][AMC_TRANSIT_COLUMNS][2], samples taken; any may be NULL; synchronises */
int amc_transit_read(amc_ctx *ctx, int64_t *totals, int64_t *n_samples);
/* the per-particle arrays of the context's range: state[hi - lo], entry[n_zones][hi - lo]; any may be NULL; synchronises */
int amc_transit_state(amc_ctx *ctx, uint32_t *state, uint32_t *entry);
/* the inverse of amc_transit_read + amc_transit_state (checkpoints); n_samples 0 .. 2^32 - 1; state == NULL: every particle
 * unknown; entry == NULL: zeros */
int amc_transit_load(amc_ctx *ctx, const int64_t *totals, int64_t n_samples, const uint32_t *state, const uint32_t *entry);
/* zero totals and n_samples, every particle unknown, clear a pending error */
int amc_transit_reset(amc_ctx *ctx);
#endif /* ARGONMC_TRANSIT_H */
