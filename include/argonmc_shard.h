/* argonmc_shard.h — the device-RNG energised pore over index-range shards: the third, small collective of the
 * sharded step and the host-free run around it.  Included by argonmc.h; the ABI version is argonmc.h's.
 *
 * The sharded device-RNG step is these calls in this order, all enqueued on the context's stream, none waiting for the host:
 *   amc_temp_begin(dt)                  drift + specular cases on [lo,hi)
 *   amc_temp_cases_device(cfg)          cases 3..9 with the device draws on [lo,hi): the draws are keyed by (particle, step,
 *                                       case, attempt), so a hit's numbers do not depend on the shard layout
 *   amc_mg_hits_pack -> all-gather #3 -> amc_mg_hits_sums(row)        the hit results of all ranks, the step's sums
 *   amc_mg_bounds                       Temp:804 on [lo,hi)
 *   amc_mg_pack -> all-gather #1 -> amc_mg_sweep, or -> amc_mg_detect -> all-gather #2 -> amc_mg_resolve
 *   amc_mg_finish(ctx, NULL)
 * Fp64 addition is order dependent and a case's hits are spread over the ranks: the hit results (particle, dp_z, dE, ok) of
 * every rank are gathered on the device and added in ascending particle index, so every rank writes the row a single
 * context's amc_temp_run_device would have written, bit for bit.
 *
 * amc_mg_hits_view: buffers of the third all-gather for `world` ranks (at most 64).  One block per rank of *block_words
 * 8-byte words: [0..6] the hits of case 3 + s on this rank, [7] unused, then per case three arrays of Hc words — particle |
 * ok << 32, dp_z, dE.  Hc = max(512, n / 2048 + 512) with n the whole system's (about five times the hits of a case and step
 * even if one shard owns them all; AMC_MG_HITS_CAP=k lowers it, AMC_MG_HITS_TILE=k the records a step is ordered in LDS, for tests).  send holds this rank's block, recv the blocks of all
 * ranks in rank order.  The pointers stay valid until the context is destroyed or the call is made with another world size.
 * amc_mg_hits_pack(world): behind amc_temp_cases_device — the rank's seven segments into its send block.
 * amc_mg_hits_sums(world, row): behind the all-gather — one workgroup of the kernel that also writes a single context's rows
 * (k_case_sums, here reading the blocks of all ranks) adds, per case, left to right from 0.0 in ascending
 * particle index over all ranks (ok == 0 skipped), folds the cases in order 3..9 and writes row `row` of the series that
 * amc_temp_series_read reads: what amc_temp_device_sums returns for the whole system.
 * A block over capacity is flagged by its owner's pack and by every rank's sums call; every rank's amc_temp_shard_run_end then
 * returns AMC_ERR_CAPACITY naming the case and the step, and no rank writes a row from truncated data.
 * The calls join the record of the sharded step (argonmc.h, "multi-GPU"); a misplaced one returns AMC_ERR_STATE before it
 * enqueues anything:
 *   amc_mg_hits_pack(world)        amc_temp_cases_device since amc_temp_begin, the hits view of `world`, no pack yet
 *   amc_mg_hits_sums(world, row)   amc_mg_hits_pack(world) of this step, no sums yet, row inside the run that was begun
 * amc_temp_begin, amc_upload, amc_init_synthetic and amc_set_shard abandon a pending hits exchange. */
#ifndef ARGONMC_SHARD_H
#define ARGONMC_SHARD_H
int amc_mg_hits_view(amc_ctx *ctx, int world, void **send, void **recv, int64_t *block_words);
int amc_mg_hits_pack(amc_ctx *ctx, int world);
int amc_mg_hits_sums(amc_ctx *ctx, int world, int64_t row);
/* The run: amc_temp_shard_run_begin sizes the series for `nsteps` rows and clears the overflow words (no step pending);
 * amc_temp_shard_run_end(nsteps done) is the run's ONE synchronisation: overflow flags, counters summed over the steps
 * (*sum, may be NULL) and n_fp_errors as amc_temp_run_device examines them; afterwards amc_temp_series_read returns the rows.
 * amc_set_step keeps its meaning.  While a surface grid is configured every such step adds the rank's own hits to its totals
 * and counts n_steps; a run that lost hits marks the surfaces as amc_temp_run_device does. */
int amc_temp_shard_run_begin(amc_ctx *ctx, int64_t nsteps);
int amc_temp_shard_run_end(amc_ctx *ctx, int64_t nsteps, amc_step_stats *sum);
#endif /* ARGONMC_SHARD_H */
