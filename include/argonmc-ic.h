/* argonmc-ic.h — overlap removal of a synthetic start on the device (opt-in).  Included by argonmc.h; the ABI
 * version is argonmc.h's (additions only).
 * (The file's name has a hyphen where the samplers' part headers have an underscore: it is no sampler, and the set of
 * argonmc_<part>.h headers is a pinned list.)
 *
 * A synthetic start (amc_init_synthetic, or the host generators of the same regions) places the atoms independently, so some
 * pairs interpenetrate at step 0.  amc_init_separate finds them with a whole-system neighbour search and redraws the atom of the
 * higher index, until no pair is left or the budget of rounds is spent.  The rule, which a host mirror reproduces exactly
 * (tests/ic_separate_ref.py):
 *   overlap   the pair (i, j), i < j, overlaps iff dx*dx + dy*dy + dz*dz < min_dist*min_dist with dx = x[i] - x[j] (dy, dz
 *             alike), evaluated left to right in IEEE double without FMA.  The comparison is strict; the rule is symmetric.
 *   loser     every j with an overlapping partner i < j.  A chain i < j < k with (i, j) and (j, k) overlapping makes j AND k
 *             losers: the set does not depend on any order.
 *   redraw    the loser j of round t >= 1 gets the position amc_init_synthetic's recipe gives for the Philox counter
 *             (j, block, t, "AMCI") under the seed: blocks 0 and 1 give u0, u1, u2, mapped to the cube, or to the cylinder of
 *             the region that holds index j (first[], radius[], z_lo[], z_hi[]), as amc_init_synthetic maps them.
 *             (amc_init_synthetic itself is round 0.)  Velocities, path accumulators and the flag are not touched.
 *   loop      t = first_round; rounds = 0
 *             repeat:  search -> P pairs, L losers
 *                      if P == 0 or rounds == max_rounds: stop
 *                      redraw the L losers with round t;  t += 1; rounds += 1
 *             max_rounds == 0 is a pure query: the overlaps are counted and nothing changes.
 * Nothing is remembered per atom between rounds and nothing depends on the cell grid, the launch geometry, the shard layout
 * or the order of anything: every rank of a sharded run that makes the same call holds the same state afterwards, and a call
 * that stopped at max_rounds, continued by a second call with first_round = next_round, equals one call with the summed budget.
 *
 * The search: the bounding box of cfg's regions (the cube; or +-max radius and min z_lo .. max z_hi) cut into
 * min(floor(extent / (min_dist * (1 + 2^-20))), AMC_IC_CELLS) (at least 1) cells per axis — AMC_IC_CELLS: an environment knob
 * read by every call, 1 .. 128, default 128 — with cell indices clamped into the box per axis, so a state with atoms outside the
 * box (an uploaded one) is still searched completely.
 *
 * cfg is amc_init_synthetic's structure: the seed and the regions (a_shape is ignored), validated as amc_init_synthetic
 * validates it.  Needs an uploaded or initialised state (else AMC_ERR_STATE).  Pending deferred results are flushed first, then
 * the kept lists and the sharded step start afresh, exactly as after amc_init_synthetic.  Returns AMC_OK whenever the loop ran:
 * pairs_left > 0 says that it did not converge, and the state is then the last round's — in region and usable.  AMC_ERR_INVALID:
 * min_dist not finite or <= 0, first_round < 1, max_rounds < 0, first_round + max_rounds beyond int32.  With n = 0 or n = 1 it
 * succeeds with zero pairs and launches nothing.  The workspace is allocated for the call and released before it returns
 * (amc_owned_count is the same before and after, also when an allocation fails).  Synchronises once per search.
 *
 * stats[8] (may be NULL): searches, rounds (redraw rounds done), redrawn (losers redrawn, summed), pairs_first, losers_first,
 *                         pairs_left, losers_left, next_round (= first_round + rounds) */
#ifndef ARGONMC_IC_H
#define ARGONMC_IC_H
#define AMC_IC_MAX_CELLS_AXIS 128   /* cells of the search box per axis, and the default of AMC_IC_CELLS */
#define AMC_IC_STATS 8
int amc_init_separate(amc_ctx *ctx, const amc_ic_config *cfg, double min_dist, int32_t first_round, int32_t max_rounds, int64_t *stats);
#endif /* ARGONMC_IC_H */
