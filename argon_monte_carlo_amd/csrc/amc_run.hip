// amc_run.hip — the step driver of libargonmc.so: what is launched for a step, and in which order.  amc_timestep and the
// amc_stage_* entry points enqueue one step (or one stage of it) and read its statistics; amc_run enqueues many under one of
// three plans — the plain sequence, the ordered workgroup on demand, the overlapped run.  Host
// code only: the kernels are in amc_stream.hip, amc_grid.hip, amc_resolve.hip and amc_clusters.hip, behind the launchers of
// amc_internal.h.  What those launchers leave pending between steps is amc_ctx::step.
#include <chrono>

#include "amc_host.h"
#include "amc_resolve_dev.h"

extern "C" {

// ---- the step ----------------------------------------------------------------------------------------------------------
static void fold_banks(amc_dev_counters *h, const amc_counter_bank *b)
{
    for (int k = 0; k < AMC_COUNTER_BANKS; k++) {
        h->n_wall += b[k].n_wall; h->n_paths += b[k].n_paths; h->n_paths_total += b[k].n_paths_total;
        h->n_fp_errors += b[k].n_fp_errors; h->n_pp += b[k].n_pp;
    }
}

// the last sweep's paths / counters are not in yet: commit it now (its results stay deferred).  An entry point that reads or
// replaces outputs calls this BEFORE its first copy or memset (amc_step_state, amc_internal.h)
int amc_settle_commit(amc_ctx *c)
{
    if (!c->step.commit_pending) return AMC_OK;
    AMC_HIP(c, amc_launch_commit(c));
    c->step.commit_pending = false;
    return AMC_OK;
}

int amc_read_counters(amc_ctx *c, amc_dev_counters *h)
{
    if (int rc = amc_settle_commit(c)) return rc;
    amc_counter_bank banks[AMC_COUNTER_BANKS];
    amc_stage st(c);
    AMC_HIP(c, st.get(h, c->d_cnt, sizeof *h));
    AMC_HIP(c, st.get(banks, c->d_banks, sizeof banks));
    AMC_HIP(c, st.finish());
    fold_banks(h, banks);
    return AMC_OK;
}

static void delta_stats(const amc_dev_counters &now, const amc_dev_counters &prev, amc_step_stats *o)
{
    o->n_pp = (int64_t)(now.n_pp - prev.n_pp);
    o->n_wall = (int64_t)(now.n_wall - prev.n_wall);
    o->n_oob_walls = (int64_t)(now.n_oob_walls - prev.n_oob_walls);
    o->n_oob_pp = (int64_t)(now.n_oob_pp - prev.n_oob_pp);
    o->n_paths = (int64_t)(now.n_paths - prev.n_paths);
    o->n_candidates = (int64_t)(now.n_candidates - prev.n_candidates);
    o->n_clusters = (int64_t)(now.n_clusters - prev.n_clusters);
    o->n_rounds = (int64_t)(now.n_rounds - prev.n_rounds);
    o->n_fp_errors = (int64_t)(now.n_fp_errors - prev.n_fp_errors);
    o->flags = (int64_t)now.flags;
}

int amc_finish_stats(amc_ctx *c, amc_step_stats *out)
{
    amc_dev_counters now;
    int rc = amc_read_counters(c, &now);
    if (rc) return rc;
    amc_step_stats st;
    delta_stats(now, c->h_prev, &st);
    c->h_prev = now;
    if (out) *out = st;
    if (now.flags & 21ULL) {    // candidate / resolve work-space / velocity-change list overflow; a full path-record buffer (bit1) only stops recording
        const unsigned long long f = now.flags;
        // clear the sticky flags on the device so that a later call can succeed after the caller drained / resized
        unsigned long long zero = 0;
        hipMemcpyAsync(&c->d_cnt->flags, &zero, sizeof zero, hipMemcpyHostToDevice, c->stream);
        hipStreamSynchronize(c->stream);
        c->h_prev.flags = 0;
        return amc_fail(c, AMC_ERR_CAPACITY, "device work buffer overflow (flags=%llu: 1 candidates, 4 resolve work space, 16 velocity changes of one step in the multi-GPU exchange)", f);
    }
    if (st.n_fp_errors > 0 && c->P.geometry != AMC_GEOM_PORE_ENERGISED && !(c->P.reserved1 & 1))
        return amc_fail(c, AMC_ERR_FP, "%lld event(s) where the reference raises FloatingPointError", (long long)st.n_fp_errors);
    return AMC_OK;
}

// sweep results deferred to the next streaming pass: write them now (before anything else reads the particle arrays)
int amc_flush(amc_ctx *c)
{
    if (int rc = amc_settle_commit(c)) return rc;       // (before the results are applied: the commit leaves the number of deferred slots)
    if (!c->step.lazy_pending) return AMC_OK;
    AMC_HIP(c, amc_launch_apply(c));
    c->step.lazy_pending = false;
    return AMC_OK;
}

int amc_enqueue_sweep(amc_ctx *c, bool counted, bool defer_commit)
{
    if (!counted) AMC_HIP(c, amc_launch_bin(c));
    AMC_HIP(c, amc_launch_detect(c));
    AMC_HIP(c, amc_launch_resolve(c, defer_commit));
    if (defer_commit) c->step.lazy_pending = true;
    return AMC_OK;
}

// fold_prev_bounds: the previous step of the same amc_run left its post-sweep bounds check to this step's streaming
// pass; defer_bounds: leave this step's to the next one (the caller runs it separately after the last step)
static int enqueue_step(amc_ctx *c, double dt, bool fold_prev_bounds = false, bool defer_bounds = false)
{
    const int g = c->P.geometry;
    int rc;
    if (g == AMC_GEOM_CELL) {
        if ((rc = amc_enqueue_sweep(c))) return rc;
    } else if (g == AMC_GEOM_CUBE || g == AMC_GEOM_PORE) {
        // the streaming pass also counts the particles into the detection grid when it covers all of them
        const bool fuse = !c->allpairs && c->lo == 0 && c->hi == c->n;
        AMC_HIP(c, amc_launch_stream(c, dt, amc_step_stages(g, fold_prev_bounds), 0, fuse));
        // the scattered commit is deferred: the next streaming pass over all particles (the bounds check for the pore,
        // the next step's drift for the cube) picks the results up through slot_of[]
        if ((rc = amc_enqueue_sweep(c, fuse, c->lo == 0 && c->hi == c->n))) return rc;
        if (g == AMC_GEOM_PORE && !defer_bounds) AMC_HIP(c, amc_launch_stream(c, dt, AMC_ST_BOUNDS, 1));
    } else {
        return amc_fail(c, AMC_ERR_INVALID, "energised walls need the host handshake: use the Python driver (amc_wall_hits/apply), or amc_temp_run_device for the device-RNG mode");
    }
    c->out.step++;
    // (a step that leaves its post-sweep bounds check to the next pass is never sampled: amc_run does not defer it)
    return amc_samplers_step(c);
}

int amc_timestep(amc_ctx *c, double dt, amc_step_stats *out)
{
    if (!c) return AMC_ERR_INVALID;
    if (!c->uploaded) return amc_fail(c, AMC_ERR_STATE, "amc_timestep before amc_upload");
    if (int rc = amc_mg_step_idle(c, "amc_timestep")) return rc;
    AMC_HIP(c, hipSetDevice(c->device));
    int rc = enqueue_step(c, dt);
    if (rc) return rc;
    return amc_finish_stats(c, out);
}

// ---- the overlapped run -----------------------------------------------------------------------------------
// Resolving a sweep is latency-bound work for a few hundred waves (k_clusters_wide, the ordered workgroup) and needs the
// PRE-sweep state; the next step's streaming pass is bandwidth- and atomic-bound work for the whole chip and needs the sweep's
// results only for the few thousand particles it touches.  Inside amc_run the two therefore run side by side: the pass reads
// the state buffer the resolve reads and writes the other one, leaves out the particles of the sweep's candidates, and a
// fix-up kernel advances those from the sweep's results afterwards (amc_stream.hip).  What is needed for it — a second set of
// state arrays and per-cell lists, the deferred-event buffers, a second stream — is allocated by the first such run.
static int ensure_overlap(amc_ctx *c)
{
    if (c->s_slab2) return AMC_OK;
    amc_alloc_group group(c);
    const size_t n = (size_t)std::max<int64_t>(c->n, 1);
    const size_t per = ((sizeof(double) * n) + 255) & ~(size_t)255;
    const size_t total = 10 * per + ((n + 255) & ~(size_t)255);
    char *slab;
    AMC_HIP(c, dalloc(c, &slab, total));
    AMC_HIP(c, hipMemsetAsync(slab, 0, total, c->stream));
    amc_state S;
    double **st[] = {&S.x, &S.y, &S.z, &S.vx, &S.vy, &S.vz, &S.d, &S.dx, &S.dy, &S.dz};
    size_t off = 0;
    for (auto pp : st) { *pp = (double *)(slab + off); off += per; }
    S.flag = (uint8_t *)(slab + off);
    S.px = c->S_buf[0].px; S.py = c->S_buf[0].py; S.pz = c->S_buf[0].pz;      // (prior_*_vals are not kept by these runs)
    const size_t nc = (size_t)c->G.ncells;
    amc_lists B = c->B_buf[1];
    AMC_HIP(c, dalloc(c, &B.rec, n + (size_t)c->max_extra));
    AMC_HIP(c, dalloc(c, &B.head, nc + 1));
    AMC_HIP(c, hipMemsetAsync(B.head, 0, sizeof(unsigned long long) * (nc + 1), c->stream));
    B.epoch = 0; B.n = (int)c->n;
    int *extra, *extra_count;
    AMC_HIP(c, dalloc(c, &extra, (size_t)2 * c->max_extra));
    AMC_HIP(c, dalloc(c, &extra_count, 2));
    AMC_HIP(c, hipMemsetAsync(extra_count, 0, 2 * sizeof(int), c->stream));
    // deferred events of a pass: wall hits (~1e-3 per particle and step in the pore), by bank
    const int cap = (int)std::max<long long>(1024, (long long)c->n / (4 * AMC_COUNTER_BANKS));
    amc_wev_rec *wev_rec;
    unsigned int *wev_count, *flags;
    AMC_HIP(c, dalloc(c, &wev_rec, (size_t)2 * AMC_COUNTER_BANKS * cap));
    AMC_HIP(c, dalloc(c, &wev_count, (size_t)2 * AMC_COUNTER_BANKS));
    AMC_HIP(c, hipMemsetAsync(wev_count, 0, sizeof(unsigned int) * 2 * AMC_COUNTER_BANKS, c->stream));
    hipStream_t stream2;
    hipEvent_t ev_detect, ev_stream;
    AMC_HIP(c, ctx_stream(c, &stream2));
    int can = 0, sync_values = c->ovl_sync_values;
    if (hipDeviceGetAttribute(&can, hipDeviceAttributeCanUseStreamWaitValue, c->device) != hipSuccess || !can) sync_values = 0;
    AMC_HIP(c, dalloc(c, &flags, 64));
    AMC_HIP(c, hipMemsetAsync(flags, 0, 64 * sizeof(unsigned int), c->stream));
    AMC_HIP(c, ctx_event(c, &ev_detect, hipEventDisableTiming));
    AMC_HIP(c, ctx_event(c, &ev_stream, hipEventDisableTiming));
    AMC_HIP(c, hipStreamSynchronize(c->stream));
    group.keep();
    c->S_buf[1] = S; c->B_buf[1] = B;
    c->extra_buf[0] = extra; c->extra_buf[1] = extra + c->max_extra; c->extra_count = extra_count;
    c->wev_buf[0] = {wev_rec, wev_count, cap};
    c->wev_buf[1] = {wev_rec + (size_t)AMC_COUNTER_BANKS * cap, wev_count + AMC_COUNTER_BANKS, cap};
    c->stream2 = stream2; c->ev_detect = ev_detect; c->ev_stream = ev_stream;
    c->ovl_sync_values = sync_values; c->ovl_flags = flags;
    c->s_slab2 = slab;          // (the guard: last)
    return AMC_OK;
}

static int run_overlapped(amc_ctx *c, double dt, int64_t nsteps)
{
    int rc = ensure_overlap(c);
    if (rc) return rc;
    if ((rc = amc_flush(c))) return rc;                 // the state is complete in the current arrays
    const int g = c->P.geometry;
    const bool two = c->overlap_mode == 1;
    int cur = (c->S.x == c->S_buf[1].x) ? 1 : 0;
    c->B_buf[cur] = c->B;                               // (the list epoch lives in the current copy)
    c->B_buf[0].extra = c->extra_buf[0]; c->B_buf[1].extra = c->extra_buf[1];
    unsigned int prev_epoch = 0;                        // the sweep in flight (none before the first step)
    for (int64_t s = 0; s < nsteps; s++) {
        const int st = amc_step_stages(g, s > 0);       // (Pore:550 of the previous step rides along)
        hipStream_t sp = two ? c->stream2 : c->stream;
        if (two) {
            // the pass may start once the previous sweep's detect kernel has marked its candidates' particles (and, at the
            // first step, once everything queued before the run has finished)
            c->ovl_tick++;
            if (c->ovl_sync_values) {
                AMC_HIP(c, hipStreamWriteValue32(c->stream, c->ovl_flags, c->ovl_tick, 0));
                AMC_HIP(c, hipStreamWaitValue32(c->stream2, c->ovl_flags, c->ovl_tick, hipStreamWaitValueGte, 0xffffffffu));
            } else {
                AMC_HIP(c, hipEventRecord(c->ev_detect, c->stream));
                AMC_HIP(c, hipStreamWaitEvent(c->stream2, c->ev_detect, 0));
            }
        }
        if (s > 0) {
            // (recorded above, BEHIND the detect kernel of step s - 1 and in front of its resolve kernels, which follow here)
            AMC_HIP(c, amc_launch_resolve(c, true));
        }
        AMC_HIP(c, amc_launch_stream_ovl(c, dt, st, cur, prev_epoch, sp, !c->overlap_split));
        if (c->overlap_split) AMC_HIP(c, amc_launch_bin_ovl(c, 1 - cur, prev_epoch, sp));
        if (two) {
            if (c->ovl_sync_values) {
                AMC_HIP(c, hipStreamWriteValue32(c->stream2, c->ovl_flags + 16, c->ovl_tick, 0));
                AMC_HIP(c, hipStreamWaitValue32(c->stream, c->ovl_flags + 16, c->ovl_tick, hipStreamWaitValueGte, 0xffffffffu));
            } else {
                AMC_HIP(c, hipEventRecord(c->ev_stream, c->stream2));
                AMC_HIP(c, hipStreamWaitEvent(c->stream, c->ev_stream, 0));
            }
        }
        AMC_HIP(c, amc_launch_fixup(c, dt, st, cur, prev_epoch));
        c->step.commit_pending = false; c->step.lazy_pending = false;             // (consumed by the fix-up kernel)
        cur = 1 - cur;
        c->S = c->S_buf[cur];
        c->B = c->B_buf[cur];
        AMC_HIP(c, amc_launch_detect(c));
        prev_epoch = c->step.sweep_epoch;
        c->out.step++;
        c->ovl_steps++;
    }
    // the last sweep: resolved, and left to the plain machinery (its commit and its results wait for the next streaming pass,
    // a flush or a read of the counters, as after any step)
    AMC_HIP(c, amc_launch_resolve(c, true));
    c->step.lazy_pending = true;
    c->step.commit_step = (int)c->out.step - 1;         // (the step index has moved on: the sweep belongs to the last step)
    c->B_buf[cur] = c->B;
    // the current lists' extra nodes die with them (the next build starts from the particles' own nodes)
    AMC_HIP(c, hipMemsetAsync(c->extra_count, 0, 2 * sizeof(int), c->stream));
    AMC_HIP(c, hipMemsetAsync(c->wev_buf[0].count, 0, sizeof(unsigned int) * 2 * AMC_COUNTER_BANKS, c->stream));
    if (g == AMC_GEOM_PORE) AMC_HIP(c, amc_launch_stream(c, dt, AMC_ST_BOUNDS, 1));     // Pore:550 of the last step
    return AMC_OK;
}

// ---- the ordered workgroup on demand -------------------------------------------------------------------------
// host state after a step has been enqueued: what a rewind to that step restores, and the arguments its wide kernel had
struct amc_od_snap {
    amc_step_state step;
    amc_lists B;
    unsigned int out_step;
    rs_args used;
};

static int run_on_demand(amc_ctx *c, double dt, int64_t nsteps)
{
    const int g = c->P.geometry;
    std::vector<amc_od_snap> ring(AMC_OD_RING);
    const int tick0 = c->od_tick;                       // step s of this run has index tick0 + s
    int rc = AMC_OK;
    // the answer to a stall: the ordered workgroup for the sweep that raised the word (it clears it), the host's epochs back
    // to the state after that step; the steps after it did nothing and are enqueued again
    auto answer = [&](int at, int64_t *s, bool stalled) -> int {
        const amc_od_snap &R = ring[at % AMC_OD_RING];
        // (the copy was taken with the step's results and commit pending and deferred; step.od_prev_ordered, false in it, is
        // set by the launch below)
        c->step = R.step; c->B = R.B; c->out.step = R.out_step;
        AMC_HIP(c, amc_launch_ordered(c, R.used));
        c->od_handled = at;
        if (stalled) { c->od_stalls++; if (at == tick0 + (int)nsteps - 1) c->od_stalls_last++; }
        *s = (int64_t)(at - tick0) + 1;
        return AMC_OK;
    };
    auto stall_seen = [&]() -> int { const int v = *c->h_od_stall; return v > c->od_handled ? v : 0; };
    c->od_active = true;
    for (int64_t s = 0;;) {
        if (s == nsteps) {
            // the end of the run: only now is it known whether a sweep before the last one still waits
            if (hipStreamSynchronize(c->stream) != hipSuccess) { rc = amc_fail(c, AMC_ERR_HIP, "hipStreamSynchronize failed in amc_run"); break; }
            int at = stall_seen();
            const bool stalled = at != 0;
            // (the last sweep gets its ordered pass in any case: the run ends in the state every other entry point expects)
            if (!at) at = tick0 + (int)nsteps - 1;
            if ((rc = answer(at, &s, stalled))) break;
            if (s == nsteps) break;
            continue;
        }
        // not more than od_ahead steps in front of the last wide kernel that ran: a stall costs the empty launches in between
        const int tick = tick0 + (int)s;
        if (tick - *c->h_od_done > c->od_ahead && !stall_seen()) {
            // (a plain read of host memory; the clock is read every 1,024 reads, and after 2 ms without a step finishing the
            // stream is asked where it is — the wait ends with the stream's completion at the latest)
            int last = *c->h_od_done;
            unsigned spins = 0;
            auto t_last = std::chrono::steady_clock::now();
            for (;;) {
                const int done = *c->h_od_done;
                if (tick - done <= c->od_ahead || stall_seen()) break;
                if (done != last) { last = done; t_last = std::chrono::steady_clock::now(); }
                else if ((++spins & 1023u) == 0 && std::chrono::steady_clock::now() - t_last > std::chrono::milliseconds(2)) {
                    if (hipStreamSynchronize(c->stream) != hipSuccess) rc = amc_fail(c, AMC_ERR_HIP, "hipStreamSynchronize failed in amc_run");
                    break;
                }
            }
            if (rc) break;
        }
        if (const int at = stall_seen()) {
            if ((rc = answer(at, &s, true))) break;
            continue;
        }
        c->od_tick = tick;
        hipError_t e = amc_launch_stream(c, dt, amc_step_stages(g, s > 0), 0, true);
        if (e == hipSuccess) e = amc_launch_detect(c);
        amc_od_snap &R = ring[tick % AMC_OD_RING];
        if (e == hipSuccess) e = amc_launch_wide_only(c, &R.used);
        if (e != hipSuccess) { rc = amc_fail(c, AMC_ERR_HIP, "launch failed in amc_run: %s", hipGetErrorString(e)); break; }
        c->step.lazy_pending = true;
        c->out.step++;
        R.step = c->step; R.B = c->B; R.out_step = c->out.step;
        s++;
    }
    c->od_active = false;
    c->od_tick = tick0 + (int)nsteps;
    if (rc) return rc;
    if (g == AMC_GEOM_PORE) AMC_HIP(c, amc_launch_stream(c, dt, AMC_ST_BOUNDS, 1));     // Pore:550 of the last step
    return AMC_OK;
}

int amc_run(amc_ctx *c, double dt, int64_t nsteps, amc_step_stats *sum)
{
    if (!c) return AMC_ERR_INVALID;
    if (!c->uploaded) return amc_fail(c, AMC_ERR_STATE, "amc_run before amc_upload");
    if (int rc = amc_mg_step_idle(c, "amc_run")) return rc;
    AMC_HIP(c, hipSetDevice(c->device));
    const bool whole = c->lo == 0 && c->hi == c->n && !c->allpairs;
    // (a sampler with a cadence, or the sampled free paths: the plain loop, whose steps end with the state a sample reads)
    const bool sampling = amc_samplers_cadence(c);
    if (c->overlap_mode && whole && nsteps >= 2 && !c->keep_prior && !c->detect_ap && c->n > 0 && !sampling &&
        (c->P.geometry == AMC_GEOM_CUBE || c->P.geometry == AMC_GEOM_PORE)) {
        int rc = run_overlapped(c, dt, nsteps);
        if (rc) return rc;
        return amc_finish_stats(c, sum);
    }
    // inside the run only the last step needs its own post-sweep bounds pass (needs the whole range in one context) — and
    // every step that is sampled: the sample sees the step's final state
    if (!c->ordered_always && whole && nsteps >= AMC_OD_MIN_STEPS && nsteps < (1 << 30) && !amc_samplers_configured(c) && !c->keep_prior && !c->detect_ap &&
        !c->d_dbg && c->n > 0 && c->n <= c->od_max_n && c->h_od_stall && c->od_tick < (1 << 30) &&
        (c->P.geometry == AMC_GEOM_CUBE || c->P.geometry == AMC_GEOM_PORE)) {
        int rc = run_on_demand(c, dt, nsteps);
        if (rc) return rc;
        return amc_finish_stats(c, sum);
    }
    const bool fold = c->P.geometry == AMC_GEOM_PORE && whole;
    bool deferred = false;
    for (int64_t s = 0; s < nsteps; s++) {
        const bool defer = fold && s + 1 < nsteps && !amc_samplers_due(c, (int64_t)c->out.step + 1);
        int rc = enqueue_step(c, dt, deferred, defer);
        if (rc) return rc;
        deferred = defer;
    }
    return amc_finish_stats(c, sum);
}

// a stage on its own starts from complete particle arrays, and is no part of a sharded step
static int stage_begin(amc_ctx *c)
{
    if (!c || !c->uploaded) return AMC_ERR_STATE;
    if (int rc = amc_mg_step_idle(c, "a stage call")) return rc;
    AMC_HIP(c, hipSetDevice(c->device));
    return amc_flush(c);
}

int amc_stage_drift(amc_ctx *c, double dt)
{
    if (int rc = stage_begin(c)) return rc;
    const bool kp = c->keep_prior;
    c->keep_prior = true;       // a following amc_stage_walls needs prior_*_vals
    hipError_t e = amc_launch_stream(c, dt, AMC_ST_DRIFT, 0);
    c->keep_prior = kp;
    AMC_HIP(c, e);
    AMC_HIP(c, hipStreamSynchronize(c->stream));
    return AMC_OK;
}

int amc_stage_walls(amc_ctx *c, amc_step_stats *out)
{
    if (int rc = stage_begin(c)) return rc;
    AMC_HIP(c, amc_launch_stream(c, 0.0, AMC_ST_WALLS, 0));
    return amc_finish_stats(c, out);
}

int amc_stage_bounds(amc_ctx *c, int64_t *n_moved)
{
    if (int rc = stage_begin(c)) return rc;
    AMC_HIP(c, amc_launch_stream(c, 0.0, AMC_ST_BOUNDS, 0));
    amc_step_stats st;
    const int rc = amc_finish_stats(c, &st);
    if (n_moved) *n_moved = st.n_oob_walls;
    return rc;
}

int amc_stage_sweep(amc_ctx *c, amc_step_stats *out)
{
    if (int rc = stage_begin(c)) return rc;
    if (int rc = amc_enqueue_sweep(c)) return rc;
    return amc_finish_stats(c, out);
}

}  // extern "C"
