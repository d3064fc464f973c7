// amc_api_mg.hip — C ABI of the multi-GPU path (one process per GPU, index-range shards): shard-local step,
// packed exchange of positions and changed velocities, then the single-GPU sweep over the whole system on every rank.
#include "amc_host.h"

extern "C" {

int amc_set_shard(amc_ctx *c, int64_t lo, int64_t hi)
{
    if (!c || lo < 0 || hi < lo || hi > c->n) return AMC_ERR_INVALID;
    c->lo = lo; c->hi = hi;
    c->MG.count_pp = (lo == 0);     // the rank that owns particle 0 reports the sweep's collision count
    amc_mg_step_fresh(c);           // (a pending pack describes the old range and the velocities published before)
    AMC_HIP(c, hipSetDevice(c->device));
    if (!c->MG.kin_vpub) AMC_HIP(c, dalloc(c, &c->MG.kin_vpub, 3 * (size_t)std::max<int64_t>(c->n, 1)));
    if (c->uploaded) return amc_publish_velocities(c);
    return AMC_OK;
}

int amc_mg_local(amc_ctx *c, double dt)
{
    if (!c || !c->uploaded) return AMC_ERR_STATE;
    if (c->allpairs || c->P.geometry == AMC_GEOM_CELL || c->P.geometry == AMC_GEOM_PORE_ENERGISED)
        return amc_fail(c, AMC_ERR_INVALID, "amc_mg_local needs the binned detector and the cube / specular pore geometry (energised walls: amc_temp_begin)");
    AMC_HIP(c, hipSetDevice(c->device));
    amc_mg_step_fresh(c);
    AMC_HIP(c, amc_launch_stream(c, dt, amc_step_stages(c->P.geometry), 0));
    return AMC_OK;
}

int amc_mg_exchange_view(amc_ctx *c, int world, void **send, void **recv, int64_t *block)
{
    if (!c || world < 1 || !send || !recv || !block) return AMC_ERR_INVALID;
    AMC_HIP(c, hipSetDevice(c->device));
    amc_mg_ws &M = c->MG;
    if (M.kin_world != world) {
        AMC_HIP(c, hipStreamSynchronize(c->stream));
        const int64_t m = std::max<int64_t>((c->n + world - 1) / world, 1);
        int64_t cap = std::max<int64_t>(4096, m / 8);
        if (const char *e = getenv("AMC_MG_VELOCITY_LIST")) { const long long v = atoll(e); if (v > 0) cap = v; }   // (tests)
        const int64_t kb = amc_kin_banks();
        cap = (cap + kb - 1) / kb * kb;                                 // the same room in every bank
        const int64_t blk = 3 * m + kb + 4 * cap;
        // kept lists (pore): a node pool per wave of the pack and of the unpack kernel, whose launch geometry is fixed by the
        // world size; the node records behind the particles' own grow if these pools need more than the single-GPU pass's
        int waves_pack = 0, waves_unpack = 0;
        size_t waves = 0, pool = 0;
        const bool kept_lists = c->keep_K >= 2 && c->B.cell_of && c->B_buf[0].rec == c->B.rec;
        if (kept_lists) {
            const int64_t per = std::max<int64_t>(m, cap);
            waves_pack = (int)((m + 255) / 256) * 4;
            waves_unpack = (int)(((int64_t)world * per + 255) / 256) * 4;
            waves = (size_t)waves_pack + (size_t)waves_unpack;
            pool = waves * (size_t)c->B.wave_cap;
        }
        const bool keep = kept_lists && (long long)c->n + (long long)pool <= 0x3fffffffLL, grow = keep && pool > c->keep_pool;
        amc_alloc_group group(c);
        double *ksend, *krecv;
        amc_rec *rec = nullptr;
        int *extra = nullptr, *wave_count = nullptr;
        AMC_HIP(c, dalloc(c, &ksend, (size_t)blk));
        AMC_HIP(c, dalloc(c, &krecv, (size_t)blk * (size_t)world));
        if (grow) AMC_HIP(c, dalloc(c, &rec, (size_t)c->n + std::max((size_t)c->max_extra, pool)));
        if (grow) AMC_HIP(c, dalloc(c, &extra, pool));
        if (keep) AMC_HIP(c, dalloc(c, &wave_count, waves));
        if (keep) AMC_HIP(c, hipMemsetAsync(wave_count, 0, sizeof(int) * waves, c->stream));
        group.keep();
        ctx_free(c, M.kin_send, M.kin_recv, M.wave_count);
        M.kin_send = ksend; M.kin_recv = krecv; M.wave_count = wave_count;
        M.kin_m = m; M.kin_cap = cap; M.kin_block = blk;
        amc_mg_step_fresh(c, true);     // (a pending pack filled the block that has just been freed)
        c->step.lists_age = -1;
        if (grow) {
            ctx_free(c, c->B.rec, c->B.extra);
            c->B.rec = rec; c->B.extra = extra; c->keep_pool = pool;
            c->B_buf[0].rec = rec; c->B_buf[0].extra = extra;
        }
        if (kept_lists) { M.waves_pack = waves_pack; M.waves_unpack = waves_unpack; }
        M.keep = keep;
        M.kin_world = world;        // (the guard: last)
    }
    *send = M.kin_send; *recv = M.kin_recv; *block = M.kin_block;
    return AMC_OK;
}

// this rank's range must be the driver's shard of that world size (the unpack side recomputes the ranges)
static int mg_check_shard(amc_ctx *c, int world, int rank)
{
    if (world != c->MG.kin_world || rank < 0 || rank >= world) return amc_fail(c, AMC_ERR_STATE, "world/rank do not match amc_mg_exchange_view");
    const int64_t base = c->n / world, rem = c->n % world;
    const int64_t lo = rank * base + std::min<int64_t>(rank, rem), hi = lo + base + (rank < rem ? 1 : 0);
    if (lo != c->lo || hi != c->hi) return amc_fail(c, AMC_ERR_STATE, "rank %d of %d owns [%lld,%lld), amc_set_shard says [%lld,%lld)", rank, world, (long long)lo, (long long)hi, (long long)c->lo, (long long)c->hi);
    return AMC_OK;
}

static const char *mg_phase_name(const amc_mg_step &s)
{
    static const char *const names[] = {"no step is pending", "amc_mg_pack is pending", "amc_mg_detect is pending", "the sweep is done: amc_mg_finish is next"};
    return names[s.phase];
}

// `who`(world) needs the pack of this step and of this world size behind it (amc_mg_step's rule)
static int mg_need_pack(amc_ctx *c, const char *who, int world)
{
    const amc_mg_step &s = c->MG.step;
    if (s.phase == AMC_MG_IDLE) return amc_fail(c, AMC_ERR_STATE, "%s(world=%d) without amc_mg_pack in this step", who, world);
    if (s.phase != AMC_MG_PACKED) return amc_fail(c, AMC_ERR_STATE, "%s(world=%d) needs a pending amc_mg_pack: %s", who, world, mg_phase_name(s));
    if (s.world != world) return amc_fail(c, AMC_ERR_STATE, "%s(world=%d) after amc_mg_pack(world=%d)", who, world, s.world);
    return AMC_OK;
}

int amc_mg_pack(amc_ctx *c, int world)
{
    if (!c || !c->uploaded) return AMC_ERR_STATE;
    amc_mg_step &s = c->MG.step;
    if (world < 1 || world != c->MG.kin_world) return amc_fail(c, AMC_ERR_STATE, "amc_mg_exchange_view(world=%d) has not been called", world);
    if (s.phase != AMC_MG_IDLE) return amc_fail(c, AMC_ERR_STATE, "amc_mg_pack(world=%d) needs a step without a pack yet: %s", world, mg_phase_name(s));
    AMC_HIP(c, hipSetDevice(c->device));
    { int rc_ = amc_flush(c); if (rc_) return rc_; }
    const int mode = amc_list_build_mode(c, 2, c->MG.keep);
    AMC_HIP(c, amc_launch_kin_pack(c, mode, !s.counts_clear));
    s.phase = AMC_MG_PACKED; s.world = world; s.mode = mode;
    s.counts_clear = false;         // (the pack kernel counts this step's velocity changes into them)
    return AMC_OK;
}

int amc_mg_sweep(amc_ctx *c, int world, int rank)
{
    if (!c || !c->uploaded) return AMC_ERR_STATE;
    if (c->allpairs || c->P.geometry == AMC_GEOM_CELL) return amc_fail(c, AMC_ERR_INVALID, "multi-GPU needs the binned detector");
    amc_mg_step &s = c->MG.step;
    if (world > 1 || s.phase != AMC_MG_IDLE) {          // (one rank, nothing packed: the lists are built below)
        if (int rc = mg_need_pack(c, "amc_mg_sweep", world)) return rc;
    }
    if (world > 1) {
        if (int rc = mg_check_shard(c, world, rank)) return rc;
    }
    AMC_HIP(c, hipSetDevice(c->device));
    { int rc_ = amc_flush(c); if (rc_) return rc_; }
    const bool lists = s.phase == AMC_MG_PACKED;
    if (world > 1) {
        AMC_HIP(c, amc_launch_kin_unpack(c, world, rank, s.mode));
        s.counts_clear = true;
    }
    // the single-GPU sweep over all n particles; the per-cell lists were built by the pack / unpack kernels (if nothing
    // was packed — one rank, no exchange — they are built here).  The scatter of the results is deferred as on one GPU:
    // the next streaming pass over the shard picks up those of its own particles, the next unpack releases the slots of
    // the others (whose results arrive from their owners).
    if (int rc = amc_enqueue_sweep(c, lists, true)) return rc;
    s.phase = AMC_MG_SWEPT;
    return AMC_OK;
}

// ---- detection sharded by index: unpack + detect over [lo, hi) | second all-gather (candidate pairs) | graph + resolve ----
int amc_mg_candidates_view(amc_ctx *c, int world, void **send, void **recv, int64_t *block_ints)
{
    if (!c || world < 1 || !send || !recv || !block_ints) return AMC_ERR_INVALID;
    AMC_HIP(c, hipSetDevice(c->device));
    amc_mg_ws &M = c->MG;
    if (M.cand_world != world) {
        AMC_HIP(c, hipStreamSynchronize(c->stream));
        // a quarter of the context's candidate capacity (n / 32 pairs by default; amc_params.max_candidates scales it): ~60x the
        // pairs a rank of eight finds per step at the reference's density, and room for the first step of a synthetic start,
        // whose uniformly placed particles overlap by the ten thousand
        long long cap = std::max<long long>(4096, c->W.max_cand / 4);
        if (const char *e = getenv("AMC_MG_CANDIDATES")) { const long long v = atoll(e); if (v > 0) cap = v; }      // (tests)
        const int cand_cap = (int)std::min<long long>(cap, c->W.max_cand);
        const size_t blk = (size_t)2 + 2 * (size_t)cand_cap;
        amc_alloc_group group(c);
        int *csend, *crecv;
        AMC_HIP(c, dalloc(c, &csend, blk));
        AMC_HIP(c, dalloc(c, &crecv, blk * (size_t)world));
        AMC_HIP(c, hipMemsetAsync(csend, 0, sizeof(int) * blk, c->stream));
        AMC_HIP(c, hipMemsetAsync(crecv, 0, sizeof(int) * blk * (size_t)world, c->stream));
        AMC_HIP(c, hipStreamSynchronize(c->stream));
        group.keep();
        ctx_free(c, M.cand_send, M.cand_recv);
        M.cand_send = csend; M.cand_recv = crecv; M.cand_cap = cand_cap;
        // (pending candidates were in the blocks that have just been freed; a pending pack is none of this view's business:
        // the driver asks for the view between the first all-gather and amc_mg_detect, dist.ShardedSimulation._sweep)
        if (M.step.phase == AMC_MG_DETECTED) amc_mg_step_fresh(c);
        M.cand_world = world;       // (the guard: last)
    }
    *send = M.cand_send; *recv = M.cand_recv; *block_ints = 2 + 2 * (int64_t)M.cand_cap;
    return AMC_OK;
}

int amc_mg_detect(amc_ctx *c, int world, int rank)
{
    if (!c || !c->uploaded) return AMC_ERR_STATE;
    if (c->allpairs || c->detect_ap || c->P.geometry == AMC_GEOM_CELL) return amc_fail(c, AMC_ERR_INVALID, "multi-GPU needs the binned detector");
    amc_mg_step &s = c->MG.step;
    if (world != c->MG.cand_world) return amc_fail(c, AMC_ERR_STATE, "amc_mg_candidates_view(world=%d) has not been called", world);
    if (int rc = mg_need_pack(c, "amc_mg_detect", world)) return rc;
    if (int rc = mg_check_shard(c, world, rank)) return rc;
    AMC_HIP(c, hipSetDevice(c->device));
    { int rc_ = amc_flush(c); if (rc_) return rc_; }
    if (world > 1) {                                    // the other shards' positions in, lists completed
        AMC_HIP(c, amc_launch_kin_unpack(c, world, rank, s.mode));
        s.counts_clear = true;
    }
    AMC_HIP(c, amc_launch_detect_own(c));
    s.phase = AMC_MG_DETECTED;
    return AMC_OK;
}

int amc_mg_resolve(amc_ctx *c, int world)
{
    if (!c || !c->uploaded) return AMC_ERR_STATE;
    amc_mg_step &s = c->MG.step;
    if (world != c->MG.cand_world) return amc_fail(c, AMC_ERR_STATE, "amc_mg_candidates_view(world=%d) has not been called", world);
    if (s.phase != AMC_MG_DETECTED) return amc_fail(c, AMC_ERR_STATE, "amc_mg_resolve(world=%d) without amc_mg_detect in this step: %s", world, mg_phase_name(s));
    if (s.world != world) return amc_fail(c, AMC_ERR_STATE, "amc_mg_resolve(world=%d) after amc_mg_detect(world=%d)", world, s.world);
    AMC_HIP(c, hipSetDevice(c->device));
    AMC_HIP(c, amc_launch_ingest(c, world));
    AMC_HIP(c, amc_launch_resolve(c, true));
    c->step.lazy_pending = true;
    s.phase = AMC_MG_SWEPT;
    return AMC_OK;
}

// ---- the hits exchange of a sharded device-RNG step: pack | third all-gather | the step's sums from all blocks (amc_hits.hip) ----
int amc_mg_hits_view(amc_ctx *c, int world, void **send, void **recv, int64_t *block_words)
{
    if (!c || world < 1 || !send || !recv || !block_words) return AMC_ERR_INVALID;
    if (world > AMC_MG_HITS_MAX_WORLD) return amc_fail(c, AMC_ERR_INVALID, "amc_mg_hits_view: %d ranks (at most %d)", world, AMC_MG_HITS_MAX_WORLD);
    AMC_HIP(c, hipSetDevice(c->device));
    amc_mg_ws &M = c->MG;
    if (M.hits_view_world != world) {
        AMC_HIP(c, hipStreamSynchronize(c->stream));
        // five times the ~n / 11,000 hits per case and step even if one shard owns them all; n is the whole
        // system's, so that all ranks agree on the block
        long long cap = std::max<long long>(512, c->n / 2048 + 512);
        if (const char *e = getenv("AMC_MG_HITS_CAP")) { const long long v = atoll(e); if (v > 0 && v < cap) cap = v; }      // (tests)
        int tile = 0x7fffffff;
        if (const char *e = getenv("AMC_MG_HITS_TILE")) { const int v = atoi(e); if (v >= 0) tile = v; }                  // (tests)
        const size_t blk = (size_t)amc_hits_block_words((int)cap);
        amc_alloc_group group(c);
        long long *hsend, *hrecv;
        int *perm;
        AMC_HIP(c, dalloc(c, &hsend, blk));
        AMC_HIP(c, dalloc(c, &hrecv, blk * (size_t)world));
        AMC_HIP(c, dalloc(c, &perm, (size_t)7 * (size_t)world * (size_t)cap));
        AMC_HIP(c, hipMemsetAsync(hsend, 0, sizeof(long long) * blk, c->stream));
        AMC_HIP(c, hipMemsetAsync(hrecv, 0, sizeof(long long) * blk * (size_t)world, c->stream));
        AMC_HIP(c, hipStreamSynchronize(c->stream));
        group.keep();
        ctx_free(c, M.hits_send, M.hits_recv, M.hits_perm);
        M.hits_send = hsend; M.hits_recv = hrecv; M.hits_perm = perm; M.hits_cap = (int)cap; M.hits_tile = tile;
        if (M.step.hits >= AMC_MG_HITS_PACKED) M.step.hits = AMC_MG_HITS_NONE;      // (the pending pack filled the block that has just been freed)
        M.hits_view_world = world;  // (the guard: last)
    }
    *send = M.hits_send; *recv = M.hits_recv; *block_words = amc_hits_block_words(M.hits_cap);
    return AMC_OK;
}

static const char *mg_hits_name(const amc_mg_step &s)
{
    static const char *const names[] = {"no device cases have been launched since amc_temp_begin", "amc_temp_cases_device is done, amc_mg_hits_pack is next",
                                        "amc_mg_hits_pack is done, amc_mg_hits_sums is next", "the hits exchange of this step is done"};
    return names[s.hits];
}

int amc_mg_hits_pack(amc_ctx *c, int world)
{
    if (!c || !c->uploaded) return AMC_ERR_STATE;
    amc_mg_step &s = c->MG.step;
    if (world < 1 || world != c->MG.hits_view_world) return amc_fail(c, AMC_ERR_STATE, "amc_mg_hits_view(world=%d) has not been called", world);
    if (s.hits != AMC_MG_HITS_LAUNCHED) return amc_fail(c, AMC_ERR_STATE, "amc_mg_hits_pack(world=%d) follows amc_temp_cases_device: %s", world, mg_hits_name(s));
    if (s.phase != AMC_MG_IDLE) return amc_fail(c, AMC_ERR_STATE, "amc_mg_hits_pack belongs in front of amc_mg_pack: %s", mg_phase_name(s));
    if (!c->TD.ovf) return amc_fail(c, AMC_ERR_STATE, "amc_mg_hits_pack without amc_temp_shard_run_begin");
    AMC_HIP(c, hipSetDevice(c->device));
    AMC_HIP(c, amc_launch_hits_pack(c));
    s.hits = AMC_MG_HITS_PACKED; s.hits_world = world;
    return AMC_OK;
}

int amc_mg_hits_sums(amc_ctx *c, int world, int64_t row)
{
    if (!c || !c->uploaded) return AMC_ERR_STATE;
    amc_mg_step &s = c->MG.step;
    if (world < 1 || world != c->MG.hits_view_world) return amc_fail(c, AMC_ERR_STATE, "amc_mg_hits_view(world=%d) has not been called", world);
    if (s.hits != AMC_MG_HITS_PACKED) return amc_fail(c, AMC_ERR_STATE, "amc_mg_hits_sums(world=%d) without amc_mg_hits_pack in this step: %s", world, mg_hits_name(s));
    if (s.hits_world != world) return amc_fail(c, AMC_ERR_STATE, "amc_mg_hits_sums(world=%d) after amc_mg_hits_pack(world=%d)", world, s.hits_world);
    if (row < 0 || row >= c->MG.hits_rows)
        return amc_fail(c, AMC_ERR_STATE, "amc_mg_hits_sums: row %lld of a run of %lld steps (amc_temp_shard_run_begin)", (long long)row, (long long)c->MG.hits_rows);
    AMC_HIP(c, hipSetDevice(c->device));
    AMC_HIP(c, amc_launch_hits_sums(c, world, row));
    s.hits = AMC_MG_HITS_SUMMED;
    return AMC_OK;
}

int amc_mg_bounds(amc_ctx *c)
{
    if (!c || !c->uploaded) return AMC_ERR_STATE;
    if (c->MG.step.phase != AMC_MG_IDLE) return amc_fail(c, AMC_ERR_STATE, "amc_mg_bounds belongs in front of amc_mg_pack: %s", mg_phase_name(c->MG.step));
    AMC_HIP(c, hipSetDevice(c->device));
    { int rc_ = amc_flush(c); if (rc_) return rc_; }
    AMC_HIP(c, amc_launch_stream(c, 0.0, AMC_ST_BOUNDS, 0));        // Temp:804 on the owned range, counters read later
    return AMC_OK;
}

int amc_mg_finish(amc_ctx *c, amc_step_stats *out)
{
    if (!c) return AMC_ERR_INVALID;
    amc_mg_step &s = c->MG.step;
    if (s.phase != AMC_MG_SWEPT) return amc_fail(c, AMC_ERR_STATE, "amc_mg_finish without amc_mg_sweep / amc_mg_resolve in this step: %s", mg_phase_name(s));
    s.phase = AMC_MG_IDLE;          // the step is over, whatever is returned below
    const bool exchanged = s.hits >= AMC_MG_HITS_PACKED;    // a sharded device-RNG step: its hits went into the surface totals
    s.hits = AMC_MG_HITS_NONE;
    AMC_HIP(c, hipSetDevice(c->device));
    if (c->P.geometry == AMC_GEOM_PORE || c->P.geometry == AMC_GEOM_PORE_ENERGISED)
        AMC_HIP(c, amc_launch_stream(c, 0.0, AMC_ST_BOUNDS, 1));                     // Pore:550 / Temp:844
    c->out.step++;
    if (exchanged && c->SF.on) c->SF.n_steps++;
    { int rc_ = amc_samplers_step(c); if (rc_) return rc_; }
    if (!out) return AMC_OK;        // asynchronous: the caller reads the counters later
    const int rc = amc_finish_stats(c, out);
    // an energised step whose work buffers overflowed: paths are missing from the sampled free paths (as after amc_temp_end)
    if (rc == AMC_ERR_CAPACITY && c->P.geometry == AMC_GEOM_PORE_ENERGISED) c->MF.lost = c->MF.on;
    return rc;
}

}  // extern "C"
