/* argonmc_mfp.h — sampled free paths: the completed free paths per spatial bin and ending kind (opt-in).
 * Included by argonmc.h; the ABI version is argonmc.h's (additions only).
 *
 * The reference's only outputs are four global free-path histograms; this sampler resolves the same paths in space and by
 * cause.  It reads the path records (amc_path_record) a step leaves on the device, so it needs them: a context created with
 * max_paths < 0 answers amc_mfp_config with AMC_ERR_STATE.  Per record:
 *   owner   the particle whose path ended: i for a wall record (phase 1..15, j == -1), which ? i : j for a p-p record
 *           (phase >= 16)
 *   kind    0: ended at a wall, 1: ended by another atom
 *   bin     the rule of the sampled fields in argonmc.h (w = (hi - lo) / n, floor((u - lo) / w), u == hi in the last bin, NaN
 *           outside; axisymmetric: r = sqrt(x*x + y*y) and z) applied to the owner's position AT THE END OF THAT STEP, read
 *           through the last sweep's deferred results.  That is within one step's flight |v| dt of the point where the path
 *           ended (about 0.07 nm at the pore's dt, about 3 nm at the cube's); a hit on an energised wall is parked at its
 *           contact point, so there it is exact.  A particle with two completed paths in one step contributes both at the
 *           same position.  An owner outside the grid only adds to n_outside (its lengths are not examined).
 * A binned record adds seven exact integers to its (bin, kind):
 *   count,  llrint(ldexp(v, 56)) for v = total, px, py, pz,  llrint(ldexp(total * total, 72)),  0 (reserved, never added to)
 * (round half to even, IEEE double as written, no FMA) and, with hist_bins > 0, one count in column h of that (bin, kind):
 *   h = amc_fields_axis(total, 0, hist_hi, hist_hi / hist_bins, hist_bins) for total < hist_hi (the rule of one axis: floor(total / w),
 *   a quotient that rounds up to hist_bins stays in the last bin), h = hist_bins ("beyond") for total >= hist_hi.
 * Valid range: all four lengths in [0, 2^-16 m) — 15 um, some 190 mean free paths at 1 atm — so that each quantised value is
 * at most 2^40; one launch handles at most 2^22 records, so its sums stay below 2^62.  They are added into signed 128-bit
 * totals (low 64 bits, high 64 bits signed); the histogram columns are plain 64-bit counts.  Everything is integer: the totals
 * do not depend on record order or launch geometry.  A binned record out of range (or NaN) stops the accumulation: its launch
 * adds nothing and no later one does, and amc_mfp_read fails with AMC_ERR_CAPACITY naming the lowest such owner
 * ("particle <index> ") until amc_mfp_reset / amc_mfp_load / amc_mfp_config.
 *
 * There is no cadence: paths are events, every completed step accumulates (amc_timestep, every step of amc_run and
 * amc_temp_run_device, amc_temp_end, amc_mg_finish) and n_steps counts them.  While a grid is configured amc_run takes its
 * plain loop and every step ends with its own bounds pass, as a sampler of the particle state with cadence 1 forces.
 * A cursor on the device marks the records already binned; after each completed step the sampler bins
 * [cursor, min(path_count, capacity)).
 *   keep_records == 0   it then empties the record buffer (path_count = 0, cursor = 0): it is the records' reader, a run of any
 *                       length works, and amc_drain_paths finds nothing while the sampler is on.
 *   keep_records == 1   the records stay for amc_drain_paths; amc_drain_paths and amc_reset_outputs zero the cursor along with
 *                       path_count (their only change, and only while a grid is configured).
 * Records consumed while an error is pending are skipped, not kept for later.  If a step leaves path_count above the
 * capacity, or more than 2^22 unseen records, records are missing: the totals are marked lost, and so they are after an
 * energised step or run that returned AMC_ERR_CAPACITY.  While lost, amc_mfp_read returns AMC_ERR_STATE until reset, load or
 * config.  amc_reset_outputs leaves totals and counters alone.  A sharded context bins the records it emitted: owners in its
 * own index range.  Without a grid every call but amc_mfp_config returns AMC_ERR_STATE, and nothing is allocated or launched. */
#ifndef ARGONMC_MFP_H
#define ARGONMC_MFP_H
#define AMC_MFP_MAX_COLUMNS 6144   /* n1 * n2 * n3 * 2 * (7 + hist_bins + 1): 48 KiB of 64-bit words, one launch's table in LDS */
#define AMC_MFP_MAX_HIST_BINS 64
typedef struct amc_mfp_grid {
    int32_t struct_size;          /* sizeof(amc_mfp_grid)                                                        */
    int32_t kind;                 /* AMC_FIELDS_CARTESIAN | AMC_FIELDS_AXISYMMETRIC (n3 == 1, lo[0] == 0)        */
    int32_t n1, n2, n3;           /* bins per axis; n1 * n2 * n3 * 2 * (7 + hist_bins + 1) <= AMC_MFP_MAX_COLUMNS */
    int32_t hist_bins;            /* 0 .. AMC_MFP_MAX_HIST_BINS columns of the per-bin histogram of `total` (+ one "beyond") */
    int32_t keep_records;         /* 0: the sampler empties the record buffer; 1: the records stay for amc_drain_paths */
    int32_t reserved;             /* 0                                                                           */
    double lo[3], hi[3];          /* as in amc_field_grid                                                        */
    double hist_hi;               /* > 0, finite: the histogram covers [0, hist_hi); unused when hist_bins == 0  */
} amc_mfp_grid;
/* NULL disables sampling and frees its memory.  A (new) grid starts from zero totals, and paths completed before the call
 * are not binned: with keep_records == 0 the call empties the record buffer (also one that has overflowed), with
 * keep_records == 1 the cursor starts at the records' current end — a buffer that has overflowed (path_count above the
 * capacity) must be drained first, or the first step marks the totals lost.  More than 2^24 particles: AMC_ERR_CAPACITY. */
int amc_mfp_config(amc_ctx *ctx, const amc_mfp_grid *grid);
/* totals[bins][2][7][2] (kinds wall, p-p; seven quantities each; words low, high), hist[bins][2][hist_bins + 1], records
 * binned, owners outside, steps completed; any may be NULL; synchronises */
int amc_mfp_read(amc_ctx *ctx, int64_t *totals, int64_t *hist, int64_t *n_records, int64_t *n_outside, int64_t *n_steps);
/* the inverse of amc_mfp_read (checkpoints); hist may be NULL when hist_bins == 0 */
int amc_mfp_load(amc_ctx *ctx, const int64_t *totals, const int64_t *hist, int64_t n_records, int64_t n_outside, int64_t n_steps);
/* zero totals and counters, clear a pending error or loss */
int amc_mfp_reset(amc_ctx *ctx);
#endif /* ARGONMC_MFP_H */
