// amc_internal.h — host-side context of libargonmc.so and the launcher prototypes shared by its translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "amc_device.h"

#define RS_SLOT_DOUBLES 12    // x y z vx vy vz d dx dy dz flag(0/1) pad  — one slot's scratch state (96 bytes)

// ---- SoA particle state in HBM (one allocation each, float64[n]; flag uint8[n]) --------------------------------
struct amc_state {
    double *x, *y, *z, *vx, *vy, *vz, *d, *dx, *dy, *dz;
    double *px, *py, *pz;     // prior_{x,y,z}_vals — written only when keep_prior is set
    uint8_t *flag;
};

// ---- detection grid: uniform cells of edge h >= collision_range, stored per z-layer inside a square xy window ---
// (the pore's body is 68 nm wide inside a 300 nm bounding box: a dense grid would be ~12x larger than needed)
struct amc_grid {
    double x0, y0, z0, h;
    double inv_h;             // cell coordinate = floor((v - v0) * inv_h): any monotone map works as long as binning
                              // and probing use the same one
    int uniform;              // 1: every layer stores the full gx*gy window (cube) -> no table lookups
    int gx, gy, gz;           // global extent in cells
    int ncells;               // stored cells = sum over layers of lay_n^2  (0 = no grid: all-pairs mode)
    double cr_probe;          // collision_range * (1 + delta): radius of every box that is probed for list entries, and
    double cr2_probe;         // its square: the distance test against a LIST RECORD's (single-precision) position.  delta
                              // covers the rounding of the records (16 x extent x 2^-24 / collision_range, at least 1e-6)
    const int *lay_lo;        // [gz] first stored cell coordinate of the window (same for x and y)
    const int *lay_n;         // [gz] window edge in cells
    const int *lay_off;       // [gz] linear offset of the layer's first cell
};

// Per-cell particle lists of the detection grid, rebuilt every step with ONE 64-bit atomic exchange per particle:
//   head[c] = (epoch << 32) | particle   — a head whose epoch is not the current one means "empty", so nothing is ever
//                                          re-zeroed and no scan / scatter pass is needed;
//   rec[p]  = (x, y, z relative to the grid origin in SINGLE precision, next particle) — 16 bytes, written coalesced
//             (indexed by the particle itself).  The records only generate candidates and validation hits — supersets,
//             re-tested exactly on the double-precision state — so half the bytes do; the particle is filed under the
//             cell of its ROUNDED position, which the detect kernel recomputes from the same record.
struct amc_rec {
    float x, y, z;
    int next;
};
#define AMC_MARK_MULTI 0xffffffffu
struct amc_lists {
    unsigned long long *head; // [ncells]
    amc_rec *rec;             // [n + max_extra]: list NODES.  Node p < n is particle p.  Nodes n + e are handed out by the fix-up
                              // kernel of an overlapped run (amc_stream.hip) to particles that had been filed under a
                              // speculative position: their own node stays linked with a position no test passes (NaN) and
                              // the particle is filed again under node n + e, extra[e] = particle
    unsigned int epoch;       // current binning epoch (>= 1)
    int n;                    // particles (nodes below n are particles themselves)
    int *extra;               // [max_extra] node n + e -> particle (nullptr: no such node exists)
    // KEPT lists (amc_list_keep, amc_grid_dev.h): the lists of a full build live on for keep_K - 1 more steps.  A
    // particle that is still in the cell it is filed under only refreshes the position in its node; one that left gives its
    // node a position no test passes (the node stays linked: walkers pass through it) and files a NEW node n + e in its new
    // cell — one atomic exchange for the ~6 % that change cell per step in the pore instead of one per particle.  Every WAVE
    // of the streaming pass has a pool of its own (64 x (keep_K - 1) nodes: each of its particles can move once per step, so
    // it cannot run out) and a counter only it touches — no atomic, no wait: read with the state, written at the end.
    int *cell_of;             // [n] cell the particle's live node is filed under
    int *node_of;             // [n] that node
    int *wave_count;          // [waves of the streaming pass] nodes the wave has handed out since the last full build
    int wave_cap;             // nodes per wave
};
#define AMC_LIST_KEEP_DEFAULT_PORE 4      // (specular pore: 126.4 against 130.8 us per step at N = 1e6, 75.5 against 77.6 at 5e5; K = 3 the same, 6 and 8 less)
#define AMC_EXTRA_NODES(n) ((int)std::min<long long>(std::max<long long>(4096, (long long)(n) / 64), 1 << 22))

// What the streaming pass of an OVERLAPPED run needs beyond the plain one (amc_run): it reads the state the
// running sweep reads (S) and writes the other buffer (S_out), leaves out every particle the sweep's detect kernel linked
// into a candidate (graph head tagged with the sweep's epoch) and defers its events (amc_out::wev).
struct amc_ovl {
    const unsigned long long *adj_head;   // nullptr: plain pass
    unsigned int skip_epoch;              // epoch of the sweep in flight (0: none)
};

// results of the last sweep that have not been written to the particle arrays yet: the next streaming pass picks them
// up (a coalesced slot_of[] read per particle) instead of a scattered commit from one workgroup
struct amc_lazy {
    int *slot_of;
    const double *state;      // [slots][RS_SLOT_DOUBLES]
    const uint8_t *moved;
    int enabled;
};

// ---- resolve scratch ---------------------------------------------------------------------------------------------
// The resolve kernels are chains of dependent, scattered accesses by a few waves: what they cost is the number of
// memory round trips and of DISTINCT arrays (every array is a base pointer to fetch and to keep in scalar registers).
// So what one thread handles at a time is ONE record (array of structures); only what the ordered workgroup scans in
// bulk stays a plain array.
// the resolve kernels' hand-over block (mirror of rs_shared in amc_resolve_dev.h)
// (Inside amc_run's on-demand loop W.ctl is STALE: it holds what the last ordered pass left — lazy_ns included — until the
// next one, and the run always ends with one.  The commit of a sweep without an ordered pass reads the wide kernel's words.)
struct amc_resolve_ctl {
    int nslots, nedges, nhist, nev, dirty, changed, nhits, nfp, ovf, nclusters, ncomplex;
    int rounds, ncand, active, ok, edges_done;
    int lazy_ns, nslots0, hist_begin, cur_round;
};
struct rs_event {             // a completed free path found by an emulation (64 bytes), emitted at commit
    int phase, i, j, which;
    long long cell;
    int slot, pad;
    double val[4];            // total, x, y, z
};
struct amc_resolve_ws {
    // candidates: cand4[k] = (i, j, next candidate in i's list, next candidate in j's list), i > j (particle indices);
    // cand_s[k] = (slot of i, slot of j, done by the wide kernel, -)
    int4 *cand4, *cand_s;
    unsigned long long *cand_mark;  // [max_cand] (sweep epoch << 32) | successor: a later candidate of this sweep shares a particle with
                              // this one — the candidate whose exchange on the particle's graph head returned this one (detect
                              // kernel); AMC_MARK_MULTI in the low half when that happened on both of its particles
    int max_cand;
    unsigned long long *adj_head;   // [n] (sweep epoch << 32) | last candidate pushed that touches the particle
    int *slot_of;             // [n] particle -> slot or -1
    unsigned int *victim;     // [n] == sweep epoch: the sweep pulled the particle into a cluster AFTER its detect kernel (it is in
                              // no candidate, so the streaming pass of an overlapped run has advanced it speculatively)
    int max_slots;
    int4 *sl_meta;            // [max_slots] (particle, cluster label at the wide kernel's hand-over, round of the last emulation, -)
    int *sl_hits;             // collisions (low half) and failed contact solves (high half) counted on the slot: atomics only
    uint8_t *sl_moved;        // the slot's scratch state differs from the particle arrays
    double *sl_state;         // [max_slots][RS_SLOT_DOUBLES]
    int *edge_a, *edge_b;     // merge edges found by validation (particles, or slots encoded as -(slot + 2))
    int max_edges;
    double4 *hist;            // position history of the sweep: (x, y, z, slot | round << 32) per new position
    int max_hist;
    int *ov_head, *ov_next;   // overlay lists of history entries per grid cell ([ncells], [max_hist])
    // Events share the index space of the history: a hit owns the entry pair (h, h + 1) — h for particle j, h + 1 for
    // particle i — and its (at most two) events sit at the same two indices; ev_gen == 0 marks "no event"
    int *ev_gen;              // [max_hist] round of the emulation that produced the event
    rs_event *ev;             // [max_hist]
    int *ctl;                 // rs_shared in global memory: hand-over between the resolve kernels
    int *wctl;                // rs_shared of the wide cluster kernel (counters it advanced before the ordered workgroup starts)
    // the ordered workgroup on demand (amc_run): where a wave of the wide kernel that leaves work for the
    // ordered workgroup says so — the sticky device word, its host-mapped mirror, the step index to write (null: nobody listens)
    int *raise_dev, *raise_host;
    int raise_tick;
    // (what only the ordered workgroup's large-sweep fallbacks touch comes last: the argument block is read line by line)
    int *sl_label, *sl_tmp;   // labels / sizes of the ordered workgroup when they do not fit its LDS
    uint8_t *sl_dirty;
    unsigned long long *sl_key;                    // sort keys (label<<32 | particle)
    int *order;
    double *cw_d[10];         // global fallback of the multi-particle clusters' working set (else LDS)
    int *cw_tmp, *cw_pidx, *cw_slot;
    uint8_t *cw_flag, *cw_moved;
};

// What the energised hand-over leaves pending between two of its calls (amc_api_temp.hip).  The rule:
//   amc_wall_hits(case)       leaves the pending hits (hits_case, hits_n, perm); it uses up ahead_case when that is `case`.
//   amc_wall_apply / _park    require hits_case == case and hits_n == n (else AMC_ERR_STATE) and clear hits_case; with n > 0 they
//                             leave ahead_case = case + 1 (-1 after case 9).  amc_wall_park also requires that nothing is parked
//                             and leaves the parked case (parked_case, parked_n, parked_perm).
//   amc_wall_finish(case, n)  requires parked_case == case and parked_n == n (else AMC_ERR_STATE) and clears parked_case.
//   amc_wall_hits_again       clears hits_case and ahead_case.
// amc_temp_begin and amc_temp_run_device start from a fresh record (fresh(): the vectors keep their capacity): a step that
// ended in an error leaves nothing behind.
// amc_temp_end returns AMC_ERR_STATE, before it enqueues anything, while a case is still parked.
struct amc_temp_handover {
    int hits_case = -1, hits_n = 0;     // the pending amc_wall_hits
    int ahead_case = -1;                // >= 0: the hits of this case are already in the records (launched behind the previous
                                        // case's apply kernel: one synchronisation serves both)
    std::vector<int> perm;              // sorted position -> record slot of the pending hits
    int parked_case = -1, parked_n = 0; // the case between amc_wall_park and amc_wall_finish
    std::vector<int> parked_perm;
    void fresh() { hits_case = ahead_case = parked_case = -1; hits_n = parked_n = 0; perm.clear(); parked_perm.clear(); }
};

// energised-wall hand-over buffers (amc_energised.hip)
struct amc_temp_ws {
    // The records live in ONE block of pinned host memory mapped into the device: the kernels write the (few hundred) hits of
    // a case straight into it and read the host's directions / energies from it — the hand-over of a case is two kernel
    // launches and two stream synchronisations, no copies.  Device addresses first, the host's view of the same bytes after.
    int *idx, *count;
    double *t, *contact, *normal, *dir, *Es, *dpz, *dE;
    unsigned char *ok;
    int *h_idx, *h_count;
    double *h_contact, *h_normal, *h_dir, *h_Es, *h_dpz, *h_dE;
    void *pin;
    int cap;
    // a PARKED case (amc_wall_park / amc_wall_finish: the gap case while its surface energies are still being integrated):
    // particle (-1: failed solve) and direction of every hit in record order, the energies / results of the finishing kernel
    int *def_idx;
    double *def_dir, *def_Es, *def_dpz, *def_dE;    // (the last three: device views of pinned memory, host views below)
    double *h_def_Es, *h_def_dpz, *h_def_dE;
    amc_temp_handover h;
};

// device-RNG mode (amc_temp_cases_device): one record segment per energised case, kept until the next step
struct temp_dev_segments {       // the segments as the kernels see them (amc_energised.hip)
    int *idx, *count;
    double *t, *contact, *normal, *dir, *Es, *dpz, *dE;
    unsigned char *ok;
    int cap;
};
// what the streaming pass's energised stage (AMC_ST_TEMP_CASES) reads besides its own arguments: in device memory, written
// once per amc_temp_run_device
struct amc_temp_pass {
    amc_temp_rng g;
    temp_dev_segments D;
};
// one row of the per-step series of a host-free run (amc_temp_run_device): what amc_temp_device_sums returns for that step
struct amc_temp_row {
    double sums[3];              // z-momentum, energy to the cold walls, energy to the hot walls
    unsigned int had;            // bit k: a hit contributed to sums[k]
    unsigned int pad;
};
struct amc_temp_dev_ws {
    temp_dev_segments seg;       // idx ... ok: [7 * cap] ([7] count), cap records per case; idx is the guard of the allocation
    // the host-free run: its series (grown when a run needs more rows), the ordering scratch of a step with more hits than
    // the sums kernel's LDS tile, the first hit-record overflow (case, row, count; case 0: none) and the pass's constants
    amc_temp_row *series;
    int64_t series_cap, series_n;
    int *perm;                   // [7 * cap]
    int *ovf;                    // [4]
    amc_temp_pass *pass;
    bool fetched;                // host copies below are valid for the last step
    int h_count[7];
    std::vector<int> h_idx[7];
    std::vector<double> h_dpz[7], h_dE[7];
    std::vector<unsigned char> h_ok[7];
};

// the bin grid of a sampler of the particle state as its kernels take it, built once at configuration (amc_sample_grid_check)
struct amc_fields_grid_dev {
    int kind, n1, n2, n3, bins; // bins = n1 * n2 * n3
    double lo[3], hi[3], w[3];  // w: bin widths (hi - lo) / n, fp64 like NumPy
};

// a moment sampler (amc_fields.hip; the sampled fields: one table of seven integers per bin, rows = 1; the sampled fluxes:
// two, rows = 2): the grid, the per-workgroup slab rows of one sample and the 128-bit running totals
struct amc_moments_ws {
    bool on;
    amc_field_grid g;           // (amc_flux_grid has the same layout)
    amc_fields_grid_dev G;
    int max_blocks;             // slab rows allocated (AMC_FIELDS_BLOCKS / AMC_FLUX_BLOCKS, else the number of CUs)
    int blocks_env;             // that knob at configuration (0: by particle count)
    unsigned long long *slab;   // [max_blocks][rows * bins * 7 + 1] one sample's sums per workgroup: row A, row B (+ particles outside)
    unsigned long long *tot;    // [bins][rows][7][2] running totals, (low, high) words
    unsigned long long *meta;   // [0] unused, [1] samples, [2] particles outside, [3] lowest particle index out of range (~0: none)
};

// sampled surfaces (amc_surface.hip): the grid, the 128-bit running totals per (case, bin, quantity) and the counters
struct amc_surface_ws {
    bool on;
    amc_surface_grid g;
    double w[AMC_SURFACE_CASES];    // bin widths (hi - lo) / nbins, fp64
    unsigned long long *tot;        // [7][nbins + 1][3][2] running totals, (low, high) words
    unsigned long long *meta;       // [0] lowest particle index out of the quantisers' range (~0: none), [1 + s] failed contact solves of case 3 + s
    int *park_bin;                  // [T.cap] bin of every record of the parked case (-1: failed contact solve), allocated at the first park
    int park_case, park_n;          // the parked case whose bins park_bin holds (0: none)
    int64_t n_steps;                // energised steps completed with the grid on
    bool lost;                      // a step or run overflowed its records: hits are missing (amc_surface_read: AMC_ERR_STATE)
};

// sampled free paths (amc_mfp.hip): the grid, the 128-bit running totals per (bin, kind, quantity), the per-bin histograms and the
// counters, the cursor among them
struct amc_mfp_ws {
    bool on;
    amc_mfp_grid g;
    amc_fields_grid_dev G;
    double hist_w;                  // hist_hi / hist_bins, fp64 (1 when hist_bins == 0)
    unsigned long long *tot;        // [bins][2][7][2] running totals, (low, high) words
    unsigned long long *hist;       // [bins][2][hist_bins + 1] counts of `total` per column, the last one "beyond"
    unsigned long long *meta;       // [0] lowest owner out of the quantisers' range (~0: none), [1] records binned, [2] owners outside,
                                    // [3] the cursor: records of the buffer already seen, [4] != 0: records were lost
    int64_t n_steps;                // steps completed with the grid on
    bool lost;                      // an energised step or run overflowed a work buffer: paths are missing (amc_mfp_read: AMC_ERR_STATE)
};

// sampled velocity distributions (amc_vdf.hip): the grid, the per-workgroup slab rows of one sample and the 64-bit running totals
struct amc_vdf_ws {
    bool on;
    amc_vdf_grid g;
    amc_fields_grid_dev G;          // the regions (bins: their number)
    int C;                          // columns per region: 4 * hist_bins + 8
    double wc, ws;                  // bin widths, fp64: 2 * v_max / hist_bins of a component, v_max / hist_bins of the speed
    int max_blocks;                 // slab rows allocated (AMC_VDF_BLOCKS, else the number of CUs)
    int blocks_env;                 // that knob at configuration (0: by particle count)
    unsigned int *slab;             // [max_blocks][regions * C + 1] one sample's counts per workgroup (+ particles outside)
    unsigned long long *tot;        // [regions][C] running totals
    unsigned long long *meta;       // [0] unused, [1] samples, [2] particles outside, [3] lowest particle index out of range (~0: none)
};

// sampled transits (amc_transit.hip): the zones, the per-particle state, the per-workgroup slab rows of one sample and the
// 128-bit running totals
struct amc_transit_ws {
    bool on;
    amc_transit_grid g;
    int max_blocks;                 // slab rows allocated (AMC_TRANSIT_BLOCKS, else the number of CUs)
    int blocks_env;                 // that knob at configuration (0: by particle count)
    int64_t stride;                 // elements per per-particle array: n rounded up to even
    unsigned int *state;            // [stride] one word per particle, four bits per zone (argonmc_transit.h), by particle index
    unsigned int *entry;            // [n_zones][stride] the sample index at which the particle was first seen inside
    unsigned long long *slab;       // [max_blocks][n_zones * 269] one sample's sums per workgroup
    unsigned long long *tot;        // [n_zones][AMC_TRANSIT_COLUMNS][2] running totals (low, high)
    unsigned long long *meta;       // [0] unused, [1] samples, [2] != 0: a sample beyond the limit was asked for, [3] lowest particle with a NaN coordinate (~0: none)
};

// sampled pair distribution (amc_pair.hip): the grid, the search cells, the records in cell order, the per-workgroup slab rows
// of one sample and the 64-bit running totals
struct amc_pair_ws {
    bool on;
    amc_pair_grid g;
    amc_fields_grid_dev G;          // the regions (bins: their number)
    amc_fields_grid_dev B;          // the search box as a Cartesian grid: lo, hi, w = the cell edges, n1 n2 n3 cells (bins: their number)
    int C;                          // columns per region: 1 + 2 * hist_bins
    double wr;                      // column width r_max / hist_bins, fp64
    int max_blocks;                 // slab rows allocated (AMC_PAIR_BLOCKS, else the number of CUs)
    int blocks_env;                 // that knob at configuration (0: one workgroup per CU)
    bool dirty;                     // a sample's launches did not all go out: cell_count and side are cleared before the next one
    unsigned int *cell_count;       // [cells] particles filed per cell; zero between samples (the scan leaves it so)
    unsigned int *cell_off;         // [cells + 1] first record of every cell, the number of records behind them
    unsigned int *wave_sum;         // [2048] the scan's sums per wave of its grid
    int *cell_of, *rank_of;         // [n] the particle's cell (-1: unfiled) and its place among the cell's records
    int2 *rec_ir;                   // [n] records in cell order: (particle index, region or -1)
    double *rec_s;                  // [6][n] ... and x y z vx vy vz
    unsigned long long *side;       // [3] one sample's particles outside and unfiled, folded into meta by the reduce (which zeroes them),
                                    // and the pair pass's work cursor (zero between samples)
    unsigned long long *slab;       // [max_blocks][regions * C] one sample's counts per workgroup
    unsigned long long *tot;        // [regions][C] running totals
    unsigned long long *meta;       // [0] the shared helpers' error word (never set: nothing is quantised), [1] samples, [2] particles outside, [3] unfiled
};

// sampled correlations (amc_corr.hip): the group grid, the window position, the origin arrays, the per-workgroup slab rows of
// one sample and the 128-bit running totals
struct amc_corr_ws {
    bool on;
    amc_corr_grid g;
    amc_fields_grid_dev G;      // the group grid (bins: the groups)
    int64_t pos;                // window position: the lag of the next sample (0: it is an origin)
    int max_blocks;             // slab rows allocated (AMC_CORR_BLOCKS, else the number of CUs)
    int blocks_env;             // AMC_CORR_BLOCKS at configuration (0: by particle count)
    int64_t stride;             // doubles per origin array (n rounded up to even: every array starts 16-byte aligned)
    double *origin;             // [6][stride] x0 y0 z0 vx0 vy0 vz0, indexed by particle like the state
    unsigned long long *slab;   // [max_blocks][2 * groups * 7 + 1] one sample's sums per workgroup (+ particles outside)
    unsigned long long *tot;    // [groups][n_lags + 1][7][2] running totals, (low, high) words
    unsigned long long *meta;   // [0] origins, [1] samples, [2] particles outside, [3] lowest particle index out of range (~0: none)
};

// What the sharded step leaves pending between two amc_mg_* calls (amc_api_mg.hip).  The rule — a call whose requirement fails
// returns AMC_ERR_STATE before it enqueues anything and leaves the record as it was:
//   amc_mg_pack(world)         requires idle and the exchange view of `world`; leaves packed(world) and `mode`.
//   amc_mg_sweep(world, rank)  world > 1: requires packed(world) and the shard check; world == 1: idle (it builds the lists
//                              itself) or packed(1).  Leaves swept.
//   amc_mg_detect(world, rank) requires packed(world), the candidates view of `world` and the shard check; leaves
//                              detected(world).
//   amc_mg_resolve(world)      requires detected(world); leaves swept.
//   amc_mg_bounds              requires idle (it moves particles: after the pack their positions have been sent); leaves idle.
//   amc_mg_finish              requires swept; leaves idle, whatever it goes on to return: the step is over.
//   amc_timestep, amc_run and the four amc_stage_* calls require idle too (amc_mg_step_idle, amc_host.h).  A step or sweep of
//                              the context's own between the pack and the unpack would run over the other shards' old
//                              positions, and — unless something flushed in between — over their slot_of[] entries of the last
//                              sweep, which only the unpack kernel releases: rs_claim_slot (amc_resolve_dev.h) would take such an
//                              index for a slot of the new sweep.
// An entry point that begins a sharded step or replaces particle state abandons what is pending (amc_mg_step_fresh below):
// amc_mg_local, amc_temp_begin, amc_temp_run_device; amc_upload, amc_init_synthetic, amc_set_shard; amc_mg_exchange_view when
// it reallocates, and amc_mg_candidates_view when it reallocates under pending candidates (detected: under a pending pack it
// changes nothing — the driver asks for it between the first all-gather and amc_mg_detect).  A later amc_mg_sweep /
// amc_mg_detect then fails ("without amc_mg_pack in this step").  The kept lists start with a full build afterwards.  What
// an abandoned pack had published is lost to the other ranks: the job recovers when every rank uploads the state again.
// Only the entry points of amc_api_mg.hip and amc_mg_step_fresh write the record; the launchers (amc_exchange.hip) are handed
// what they need and report nothing back through the context.
// The hits exchange of a sharded device-RNG step (amc_hits.hip) is part of the same record, beside the phase:
//   amc_temp_cases_device      leaves hits = launched (the one writer outside amc_api_mg.hip: it completes the segments).
//   amc_mg_hits_pack(world)    requires launched and the hits view of `world`; leaves packed(world).  A second pack is refused.
//   amc_mg_hits_sums(world, row)   requires packed(world) and a row of the run begun by amc_temp_shard_run_begin; leaves summed.
//   amc_mg_finish              clears it (and counts the step for the sampled surfaces when the exchange took place).
// amc_mg_step_fresh abandons a pending hits exchange with everything else: amc_temp_begin, amc_upload, amc_set_shard.
enum amc_mg_phase { AMC_MG_IDLE = 0, AMC_MG_PACKED, AMC_MG_DETECTED, AMC_MG_SWEPT };
enum amc_mg_hits_phase { AMC_MG_HITS_NONE = 0, AMC_MG_HITS_LAUNCHED, AMC_MG_HITS_PACKED, AMC_MG_HITS_SUMMED };
#define AMC_MG_HITS_MAX_WORLD 64   // ranks whose segment offsets fit the LDS table of k_case_sums over the blocks (amc_hits.hip)
struct amc_mg_step {
    amc_mg_phase phase;            // (zero: idle)
    amc_mg_hits_phase hits;        // (zero: none)
    int hits_world;                // the world size of the pending hits pack
    int world;                     // the world size of the pending pack (packed, detected)
    int mode = 1;                  // this step's list build: 1 anew, 2 full build of a kept cycle, 3 a step in between — written by
                                   // the pack, read by the unpack
    bool counts_clear;             // the bank counters in kin_send are zero (the unpack kernel clears them for the next pack)
    void fresh() { phase = AMC_MG_IDLE; counts_clear = false; }     // (costs the next pack one 128-byte memset)
};

// multi-GPU (amc_api_mg.hip, amc_exchange.hip)
struct amc_mg_ws {
    bool count_pp = true;          // this rank adds the p-p collision count to its counters
    double *kin_send, *kin_recv;   // per-step exchange (amc_exchange.hip): one block of kin_block doubles, and world of them
    double *kin_vpub;              // [3][n] velocities as last published to the other ranks (allocated by amc_set_shard;
                                   // every upload publishes: all ranks upload the same full state)
    int kin_world;
    int64_t kin_m, kin_cap, kin_block;   // shard length (padded), capacity of the velocity-change list (all banks), 3m + banks + 4cap
    int *cand_send, *cand_recv;    // detection sharded by index: this rank's candidate block ([0] count, [2 + 2k] pairs)
    int cand_cap, cand_world;      // and the blocks of all ranks (the second all-gather of a step); pairs per block
    // kept lists in the exchange kernels (pore, amc_lists): pools per wave of the pack and of the unpack kernel
    int *wave_count;               // [waves_pack + waves_unpack]
    int waves_pack, waves_unpack;
    bool keep;                     // the pools exist for the current world size
    // the hits exchange of a sharded device-RNG step (amc_hits.hip): this rank's block, the blocks of all ranks, the ordering
    // scratch of a step with more records than the sums kernel's LDS tile; hits_cap records per case and rank
    long long *hits_send, *hits_recv;
    int *hits_perm;                // [7 * world * hits_cap]
    int hits_cap, hits_view_world;
    int hits_tile;                 // records up to which the sums kernel orders a step in LDS (AMC_MG_HITS_TILE, else its whole tile)
    int64_t hits_rows;             // rows of the series the run in progress may write (amc_temp_shard_run_begin; 0: none)
    amc_mg_step step;
};

// what amc_ctx::owned records (amc_host.h): the context's device / pinned allocations, streams and events
enum amc_res_kind { AMC_RES_DEVICE, AMC_RES_PINNED, AMC_RES_STREAM, AMC_RES_EVENT };
struct amc_res { void *p; amc_res_kind kind; };

#define AMC_OD_AHEAD 2          // default of amc_ctx::od_ahead (experiments: environment variable AMC_OD_AHEAD)
#define AMC_OD_MAX_N 100000     // default of amc_ctx::od_max_n: measured faster at N = 1e5, slower at N = 1e6 (AMC_OD_MAX_N)
#define AMC_OD_RING 64          // snapshots kept (od_ahead is capped at 32)
#define AMC_OD_MIN_STEPS 8      // shorter runs keep the ordered workgroup in every sweep (the run ends with a synchronisation of its own)
#define AMC_PLAN_SMALL 430      // default of amc_ctx::plan_small: measured crossover of the two launch plans (tools/plan_sweep.sh;
                                // experiments: environment variable AMC_PLAN_SMALL)
#define AMC_CW_DENSE_MAX 256    // default of amc_ctx::cw_dense_max: the largest of 0 / 256 / 512 / 1024 / 2048 at which the dense scan of the
                                // wide kernel's validation was not slower than the overlay lists at N = 1e5, 3e5 and 5e5 (DESIGN.md 7,
                                // profiles/r21_ab_wide_dense.json; environment variable AMC_CW_DENSE_MAX, 0 = lists always)

// What the launchers change as they enqueue a step: everything a rewind of amc_run's on-demand loop has to put back (it keeps
// a copy per step, together with c->B and c->out.step).  A new per-step member of the host's goes HERE.
// (What the SHARDED step leaves pending between two amc_mg_* calls is amc_mg_step, amc_ctx::MG.step: amc_run requires an idle
// one and never touches it, so a rewind has nothing of it to put back.)
// The rule for what a step leaves pending: an entry point that reads outputs runs the pending commit before its first copy
// (amc_settle_commit, or amc_read_counters which starts with it); one that reads or replaces particle arrays calls amc_flush
// first; amc_reset_outputs runs the pending commit and then zeroes, and leaves lazy_pending alone.
struct amc_step_state {
    bool lazy_pending;             // sweep results wait in the slot arrays for the next streaming pass (or amc_flush)
    bool commit_pending;           // the last sweep's commit (paths -> histograms, counters, overlay) waits for the next streaming pass (or amc_flush)
    bool commit_defer;             // ... and that sweep's results stay in the slot arrays
    int commit_step = 0;           // ... and the `step` key its path records carry: the index of the sweep's own step, whoever commits it
    unsigned int sweep_epoch;      // tag of the degree counts of the current sweep (advanced by every detect launch)
    bool plan_split;               // launch plan of the current sweep, fixed when its detect kernel is launched
    int lists_age = -1;            // steps since the last full build of a kept cycle (-1: the lists are not a kept cycle's)
    int lists_owner;               // who runs the cycle: 1 the streaming pass, 2 the multi-GPU exchange kernels (their node pools differ)
    bool od_prev_ordered = true;   // the last sweep had its ordered pass: W.ctl holds its counts (else the wide kernel's words do)
    int64_t full_builds = 0;       // full builds of a kept cycle since amc_create (amc_lists_stats; a rewound step takes its own back)
};

// Created by amc_create with value-initialisation: every member without an initialiser below starts at zero.
struct amc_ctx {
    amc_params P;
    int device;
    hipStream_t own_stream, stream;
    std::string err;
    int64_t n, lo, hi;
    bool uploaded;
    bool keep_prior;
    std::vector<amc_res> owned;    // everything allocated for the context, in order (amc_host.h); amc_destroy frees it
    amc_step_state step;
    // particle state, detection grid, per-cell lists
    amc_state S;              // the CURRENT state arrays (one of S_buf's two sets)
    char *s_slab;             // the one allocation the particle state arrays are carved from
    amc_grid G;
    std::vector<int> h_lay_lo, h_lay_n, h_lay_off;
    int *d_lay;               // device copy of the three layer tables, contiguous
    amc_lists B;              // the CURRENT per-cell lists (one of B_buf's two)
    int max_extra;            // list nodes behind the particles' own that an overlapped run's fix-up kernel may hand out
    int keep_K;               // kept lists: a full build every keep_K steps (< 2: every step, the lists are not kept)
    size_t keep_pool;         // nodes behind the particles' own in B.rec / entries of B.extra
    bool allpairs;            // no detection grid at all (single cells, N <= 4096): all-pairs detector, brute-force validation
    bool detect_ap;           // candidates come from the LDS-tiled all-pairs kernel (always without a grid; with one when detect_mode == 2)
    // the sweep
    amc_resolve_ws W;
    char *w_slab;             // the one allocation W's arrays are carved from
    volatile int *h_host_ncand;    // host-mapped word written by k_resolve (candidate count of the last sweep)
    int *d_host_ncand;             // its device address
    amc_temp_ws T;
    amc_temp_dev_ws TD;
    amc_wall_law wall_law = {}; // the device-RNG steps' wall law (amc_temp_wall_law; struct_size 0: never set, the reference law)
    amc_moments_ws F;           // the sampled fields
    amc_surface_ws SF;
    amc_corr_ws CR;
    amc_moments_ws FX;          // the sampled fluxes
    amc_mfp_ws MF;              // the sampled free paths
    amc_vdf_ws VD;              // the sampled velocity distributions
    amc_transit_ws TR;          // the sampled transits
    amc_pair_ws PD;             // the sampled pair distribution
    // outputs
    amc_out out;
    amc_path_record *d_rec;
    unsigned long long *d_hist;
    double *d_edges;
    amc_dev_counters *d_cnt;
    amc_counter_bank *d_banks;   // banked per-event counters, folded into the copy read_counters() returns
    amc_dev_counters h_prev;  // snapshot used to report per-step deltas
    long long *d_dbg;         // resolve phase timers (diagnostic, enabled by AMC_DEBUG_RESOLVE=1)
    // pinned host staging for the small per-step read-backs (a copy into pageable memory costs ~100 us on this stack)
    char *h_pin;
    size_t h_pin_bytes;
    // environment switches, read once by amc_create (amc_api.hip)
    int overlap_mode;         // AMC_OVERLAP: 0 off (default), 1 two streams, 2 the same kernels in order on one stream (debug)
    bool overlap_split;       // AMC_OVERLAP_SPLIT != 0: an overlapped run builds its lists in a kernel of its own
    int cw_blocks_env;        // AMC_CW_BLOCKS (0 = default number of wide-kernel waves)
    int cw_dense_max = AMC_CW_DENSE_MAX;   // AMC_CW_DENSE_MAX: candidates up to which a sweep's new positions are validated by a dense scan (0: lists always)
    int stream_bs;            // AMC_STREAM_BS: block size of the streaming pass (the kept-list pools are sized for it)
    int detect_bs;            // AMC_DETECT_BS: block size of the list-based detect kernel
    bool temp_unfused;        // AMC_TEMP_UNFUSED set: the device-RNG energised mode runs one kernel triple per case
    bool temp_run_unfused;    // amc_temp_run_device enqueues the three streaming passes of a single step (AMC_TEMP_RUN_UNFUSED / _FUSED)
    bool ordered_always;      // AMC_ORDERED_ALWAYS != 0: k_resolve<GEOM,0> in every sweep, as amc_timestep does
    int64_t od_max_n = AMC_OD_MAX_N;   // AMC_OD_MAX_N: particle counts above this keep the ordered workgroup in every sweep
    int od_ahead = AMC_OD_AHEAD;   // AMC_OD_AHEAD: steps amc_run may be ahead of the last step the GPU has started to resolve
    int plan_small = AMC_PLAN_SMALL;   // AMC_PLAN_SMALL: candidate pairs up to which the single resolve kernel does the whole sweep
    long long allpairs_max_n; // AMC_ALLPAIRS_MAX_N: cube / pore contexts up to this size run without the detection grid (0: none)
    int list_keep;            // AMC_LIST_KEEP, else the geometry's default: the kept-list cycle asked for (amc_create caps it: keep_K)
    int max_hist_env;         // AMC_MAX_HIST (diagnostic): history entries a sweep may use (0: all that are allocated)
    bool debug_resolve;       // AMC_DEBUG_RESOLVE set: d_dbg is allocated
    // profiling
    bool profiling;
    double k_ms[AMC_K_COUNT];
    int64_t k_launches[AMC_K_COUNT];
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
    std::vector<std::pair<int, int>> ev_pending;   // (kernel class, pool index)
    size_t ev_used;
    hipEvent_t prof_ev0, prof_ev1;  // the open bracket's events (nullptr outside a bracket / when not profiling): AMC_LAUNCH
                                    // attaches them to the dispatch itself
    // the overlapped run (amc_run.hip)
    amc_state S_buf[2];       // [1] is allocated by the first overlapped run: its streaming pass writes the buffer the sweep in
    char *s_slab2;            // flight does not read
    amc_lists B_buf[2];
    int *extra_buf[2];        // node -> particle of the extra nodes of each list buffer, and how many were handed out
    int *extra_count;         // [2]
    amc_wev wev_buf[2];       // deferred events of the overlapped streaming pass, by step parity
    hipStream_t stream2;      // the overlapped streaming pass runs here
    hipEvent_t ev_detect, ev_stream;
    unsigned int *ovl_flags;  // two words (64 bytes apart) the streams of an overlapped run signal each other through
    unsigned int ovl_tick;    // (AMC_OVERLAP_SYNC=value: hipStreamWriteValue32 / hipStreamWaitValue32 instead of event record + wait —
    int ovl_sync_values;      // ~2 us per dependency instead of ~8, tools/ubench_xstream.hip, but the resolve suffers more: DESIGN 4.2)
    int64_t ovl_steps;        // steps run overlapped so far
    // The ordered workgroup on demand (amc_run.hip): steps are enqueued without k_resolve<GEOM,0>; a
    // sweep that needs it sets the sticky device word `stalled_at` to its step index, every kernel of a later step then leaves
    // without a side effect, and the host — which watches the host-mapped mirror — launches the workgroup for that sweep and
    // enqueues the later steps again.
    int *d_od;                     // [0] stalled_at (0: none)
    volatile int *h_od_stall, *h_od_done;   // host-mapped: mirror of stalled_at, step index of the last wide kernel that ran
    int *d_od_stall_host, *d_od_done_host;  // their device addresses
    bool od_active;                // the launchers pass the word and the step index (inside amc_run's on-demand loop only)
    int od_tick = 1;               // step index of the step being enqueued (never 0, grows across runs)
    int od_handled;                // the last stall the host has answered
    int64_t od_ordered_launches;   // launches of k_resolve<GEOM,0> so far
    int64_t od_steps;              // steps enqueued without it
    int64_t od_stalls, od_stalls_last;   // stalls the host has answered; those raised by the last step of their run
    amc_mg_ws MG;                  // multi-GPU (amc_api_mg.hip, amc_exchange.hip)
};

// Abandon what the sharded step has pending (the rule above amc_mg_step): the one call of every entry point named there.
// An idle record stays as it is — after a completed step the unpack kernel has cleared the bank counters, so a correct run
// enqueues no memset of them.  send_replaced: the send block is a new allocation, whatever the phase.
static inline void amc_mg_step_fresh(amc_ctx *c, bool send_replaced = false)
{
    if (!send_replaced) c->MG.step.hits = AMC_MG_HITS_NONE;     // (a pending hits exchange goes with it; a new send block of
                                                                // the position exchange and the lists are none of its business)
    if (!send_replaced && c->MG.step.phase == AMC_MG_IDLE) return;
    c->MG.step.fresh();
    c->step.lists_age = -1;         // (an abandoned pack may have begun a kept cycle with its own shard only)
}

int amc_fail(amc_ctx *c, int code, const char *fmt, ...);
#define AMC_HIP(c, call)                                                                                      \
    do {                                                                                                      \
        hipError_t e__ = (call);                                                                              \
        if (e__ != hipSuccess) return amc_fail((c), AMC_ERR_HIP, "%s failed: %s (%s:%d)", #call,             \
                                               hipGetErrorString(e__), __FILE__, __LINE__);                   \
    } while (0)

// Every kernel of the step is launched through AMC_LAUNCH.  Inside an open profiling bracket the launch carries the
// bracket's two events ON THE DISPATCH (hipExtLaunchKernelGGL: start = the kernel begins to execute, stop = it has
// finished) — the same begin / end timestamps rocprofv3 --kernel-trace reports, so bench.py's per-kernel figures agree
// with the committed kernel statistics and their sum stays below the step time (events recorded around a launch with
// hipEventRecord also count the dispatch gap in front of it: 2-4 us per kernel, which made the classes of the round-2
// line add up to more than the step).  Outside a bracket both events are null: a plain launch.
#define AMC_LAUNCH(c, kernel, grid, block, ...) \
    hipExtLaunchKernelGGL(kernel, grid, block, 0, (c)->stream, (c)->prof_ev0, (c)->prof_ev1, 0, __VA_ARGS__)
#define AMC_LAUNCH_ON(c, stream_, kernel, grid, block, ...) \
    hipExtLaunchKernelGGL(kernel, grid, block, 0, stream_, (c)->prof_ev0, (c)->prof_ev1, 0, __VA_ARGS__)

// profiling brackets
void amc_prof_begin(amc_ctx *c, int kclass);
void amc_prof_end(amc_ctx *c);
void amc_prof_cancel(amc_ctx *c);
void amc_prof_collect(amc_ctx *c);

// stage bits of the streaming kernel
#define AMC_ST_DRIFT 1
#define AMC_ST_WALLS 2
#define AMC_ST_BOUNDS 4
#define AMC_ST_BOUNDS_PRE 8     // the PREVIOUS step's bounds check after its sweep (Pore:550), folded into this pass
#define AMC_TEMP_RUN_FUSED_DEFAULT 1   // amc_temp_run_device: one fused streaming pass per step unless AMC_TEMP_RUN_UNFUSED=1
#define AMC_ST_TEMP_CASES 16    // energised pore, device-RNG mode: cases 3-9 (Temp:705-758) between the walls and the bounds check
// the stages of a cube / specular-pore step's streaming pass; prev_bounds: the previous step's post-sweep bounds check rides along
static inline int amc_step_stages(int geometry, bool prev_bounds = false)
{
    if (geometry == AMC_GEOM_CUBE) return AMC_ST_DRIFT | AMC_ST_WALLS;
    return AMC_ST_DRIFT | AMC_ST_WALLS | AMC_ST_BOUNDS | (prev_bounds && geometry == AMC_GEOM_PORE ? AMC_ST_BOUNDS_PRE : 0);
}

// launchers (each enqueues on c->stream; returns hipError_t of the launch)
hipError_t amc_launch_stream(amc_ctx *c, double dt, int stages, int bounds_slot, bool fuse_bin = false);
// (stages with AMC_ST_TEMP_CASES: the caller has written c->TD.pass and cleared the segments' counters)
// the overlapped run (amc_stream.hip): the streaming pass of the next step while the sweep is being resolved,
// and the fix-up kernel that joins the two
hipError_t amc_launch_stream_ovl(amc_ctx *c, double dt, int stages, int from, unsigned int skip_epoch, hipStream_t stream,
                                 bool build_lists = true);
hipError_t amc_launch_fixup(amc_ctx *c, double dt, int stages, int from, unsigned int sweep_epoch);
hipError_t amc_launch_bin_ovl(amc_ctx *c, int to, unsigned int skip_epoch, hipStream_t stream);
int amc_list_build_mode(amc_ctx *c, int owner, bool kept);     // this step's list build for `owner`: 1 anew, 2 / 3 kept cycle (amc_stream.hip)
hipError_t amc_launch_bin(amc_ctx *c);                 // stand-alone list build over all n particles (stages, multi-GPU)
hipError_t amc_launch_detect(amc_ctx *c);              // binned or all-pairs, fills W.cand_* / counters.cand_count
hipError_t amc_launch_detect_own(amc_ctx *c);          // multi-GPU: own index range against everybody, into the candidate block
hipError_t amc_launch_ingest(amc_ctx *c, int world);   // ... and the candidate graph from the gathered blocks of all ranks
hipError_t amc_launch_resolve(amc_ctx *c, bool defer_commit = false);   // resolve_A -> validate -> resolve_B -> commit
struct rs_args;
hipError_t amc_launch_wide_only(amc_ctx *c, rs_args *used);     // on demand: k_clusters_wide alone (results deferred); the arguments it used
hipError_t amc_launch_ordered(amc_ctx *c, const rs_args &used);  // ... and k_resolve<GEOM,0> for that sweep, later
hipError_t amc_launch_apply(amc_ctx *c);                // write deferred sweep results to the particle arrays now
hipError_t amc_launch_commit(amc_ctx *c);               // the pending commit as a kernel of its own
struct amc_commit_args;
amc_commit_args amc_make_commit_args(amc_ctx *c);       // amc_stream.hip
hipError_t amc_launch_temp_hits(amc_ctx *c, int case_id);
hipError_t amc_launch_temp_apply(amc_ctx *c, int case_id, int n, bool park = false);
hipError_t amc_launch_temp_velocity(amc_ctx *c, int case_id, int n);
hipError_t amc_launch_temp_cases_device(amc_ctx *c, const amc_temp_rng *cfg);
// the wall law of the context's device-RNG steps (amc_temp_wall_law): its kind, and the parameters its kernels are launched with
inline int amc_wall_law_kind(const amc_ctx *c) { return c->wall_law.struct_size ? c->wall_law.kind : AMC_WALL_LAW_REFERENCE; }
amc_params amc_wall_law_params(const amc_ctx *c);
hipError_t amc_launch_temp_sums(amc_ctx *c, int64_t row);     // the step's sums -> row `row` of the series (one workgroup)
// sampled surfaces (amc_surface.hip; callers test c->SF.on first): the records of all seven segments of a device-RNG step, of
// the hand-over's current case, and the two halves of a parked case
hipError_t amc_launch_surface_device(amc_ctx *c);
hipError_t amc_launch_surface_case(amc_ctx *c, int case_id, int n);
int amc_surface_park(amc_ctx *c, int case_id, int n);             // (allocates park_bin at the first call: an amc_status)
hipError_t amc_launch_surface_finish(amc_ctx *c, int case_id, int n);
// the samplers' reduce (amc_fields.hip): `rows` slab rows of `tables` tables of M sums (+ the particles outside) into the 128-bit
// totals [M / 7][lags1][7][2] at lag_a (table 0) and lag_b (table 1), counters in meta ([0] += origin, [1] += 1, [2] += outside)
hipError_t amc_launch_sample_reduce(amc_ctx *c, const unsigned long long *slab, int rows, int M, int tables, int lag_a, int lag_b,
                                    int lags1, int origin, unsigned long long *tot, unsigned long long *meta);
// the exchange kernels (amc_exchange.hip): they read c->MG and change nothing in it.  clear_counts: zero the send block's bank
// counters in front of the pack kernel
hipError_t amc_launch_kin_pack(amc_ctx *c, int mode, bool clear_counts);
hipError_t amc_launch_kin_unpack(amc_ctx *c, int world, int rank, int mode);
int amc_kin_banks(void);
// the hits exchange of a sharded device-RNG step (amc_hits.hip): they read c->MG / c->TD and change nothing in them
int64_t amc_hits_block_words(int hits_cap);
hipError_t amc_launch_hits_pack(amc_ctx *c);
hipError_t amc_launch_hits_sums(amc_ctx *c, int world, int64_t row);         // banks of the velocity-change list in an exchange block
