// amc_api.hip — the C ABI of libargonmc.so (include/argonmc.h): context, HBM allocation, upload/download, outputs and
// measurement helpers (the step driver: amc_run.hip).  No CPU compute path exists here: without a HIP device amc_create fails.
#include <memory>
#include <type_traits>

#include "amc_host.h"

int amc_fail(amc_ctx *c, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    return code;
}

static thread_local std::string g_create_err;

// ---- profiling brackets ---------------------------------------------------------------------------------------------
void amc_prof_begin(amc_ctx *c, int kclass)
{
    if (!c->profiling) return;
    if (c->ev_used == c->ev_pool.size()) {
        hipEvent_t a, b;
        (void)ctx_event(c, &a, hipEventDefault);
        (void)ctx_event(c, &b, hipEventDefault);
        c->ev_pool.push_back({a, b});
    }
    c->ev_pending.push_back({kclass, (int)c->ev_used});
    // the launch inside the bracket takes the two events with it (AMC_LAUNCH)
    c->prof_ev0 = c->ev_pool[c->ev_used].first;
    c->prof_ev1 = c->ev_pool[c->ev_used].second;
}
void amc_prof_end(amc_ctx *c)
{
    if (!c->profiling) return;
    c->prof_ev0 = c->prof_ev1 = nullptr;
    c->ev_used++;
    if (c->ev_used >= 4096) amc_prof_collect(c);
}
void amc_prof_cancel(amc_ctx *c)        // drop the open bracket (nothing was launched inside it)
{
    if (!c->profiling || c->ev_pending.empty()) return;
    c->ev_pending.pop_back();
    c->prof_ev0 = c->prof_ev1 = nullptr;
}
void amc_prof_collect(amc_ctx *c)
{
    if (!c->profiling || c->ev_pending.empty()) return;
    hipStreamSynchronize(c->stream);
    for (auto &pr : c->ev_pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, c->ev_pool[pr.second].first, c->ev_pool[pr.second].second) == hipSuccess) {
            c->k_ms[pr.first] += ms;
            c->k_launches[pr.first]++;
        }
    }
    c->ev_pending.clear();
    c->ev_used = 0;
}

// ---- helpers ------------------------------------------------------------------------------------------------------------
static int next_pow2(int v)
{
    int m = 1;
    while (m < v) m <<= 1;
    return m;
}

// detection grid: uniform cells, per-layer square window (full extent in the open-air end caps, gap radius inside
// the pore body); Cube: one window for all layers
static int setup_grid(amc_ctx *c)
{
    const amc_params &P = c->P;
    amc_grid &G = c->G;
    memset(&G, 0, sizeof G);
    if (c->allpairs) return AMC_OK;
    const double cr = P.collision_range;
    double xlo, xhi, zlo, zhi, volume;
    if (P.geometry == AMC_GEOM_CUBE) {
        xlo = 0; xhi = std::max(P.cube_x, P.cube_y); zlo = 0; zhi = P.cube_z;
        volume = P.cube_x * P.cube_y * P.cube_z;
    } else {
        xlo = -P.R_oa; xhi = P.R_oa; zlo = 0; zhi = P.H;
        const double pi = 3.14159265358979323846;
        volume = 2 * pi * P.R_oa * P.R_oa * P.h_oa + pi * P.R_g * P.R_g * (P.H - 2 * P.h_oa);
    }
    // list records hold positions relative to the grid origin in single precision: every test against them, and every box
    // that selects the cells to probe, is widened by 16 roundings of the largest coordinate (guard cells included)
    const double extent = 1.05 * std::max(xhi - xlo, zhi - zlo) + 8 * cr;
    const double delta = std::max(1.0e-6, 16.0 * extent * 5.9604644775390625e-08 / cr);
    const double crp = cr * (1.0 + delta);
    double h = P.fine_cell;
    if (!(h > 0)) {
        const double spacing = cbrt(volume / (double)std::max<int64_t>(1, c->n));
        // ~0.25 particles per cell: short lists (each further list element is a dependent random access) against more
        // cells per probe box; measured optimum on MI355X between 0.5 and 0.7 of the mean spacing
        h = std::max(0.63 * spacing, 2.01 * crp);
    }
    // probes look at the cells overlapped by a +-collision_range box: at most 2 per axis needs h >= 2*collision_range
    if (h < 2.00001 * crp) return amc_fail(c, AMC_ERR_INVALID, "fine_cell %g must be at least 2x the probe radius %g (collision_range %g widened for the single-precision list records)", h, crp, cr);
    // keep the table bounded
    for (;;) {
        const double nxy = ceil((xhi - xlo) / h) + 2, nz = ceil((zhi - zlo) / h) + 2;
        if (nxy * nxy * nz < 2.0e8) break;
        h *= 1.26;
    }
    G.h = h;
    G.inv_h = 1.0 / h;
    G.cr_probe = crp;
    G.cr2_probe = crp * crp;
    G.uniform = (P.geometry == AMC_GEOM_CUBE) ? 1 : 0;
    G.x0 = xlo - h; G.y0 = xlo - h; G.z0 = zlo - h;           // one guard cell on every side
    G.gx = G.gy = (int)ceil((xhi - xlo) / h) + 2;
    G.gz = (int)ceil((zhi - zlo) / h) + 2;
    c->h_lay_lo.assign(G.gz, 0);
    c->h_lay_n.assign(G.gz, G.gx);
    c->h_lay_off.assign(G.gz, 0);
    if (P.geometry != AMC_GEOM_CUBE) {
        // pore body layers only need |x|,|y| <= R_g (+ one guard cell); layers touching the end caps keep the full disc
        const double body_lo = P.h_oa + h + cr, body_hi = P.z_cold - h - cr;
        const int w_lo = std::max(0, (int)floor((-P.R_g - cr - G.x0) / h) - 1);
        const int w_hi = std::min(G.gx - 1, (int)floor((P.R_g + cr - G.x0) / h) + 1);
        for (int k = 0; k < G.gz; k++) {
            const double z_a = G.z0 + k * h, z_b = z_a + h;
            if (z_a > body_lo && z_b < body_hi) { c->h_lay_lo[k] = w_lo; c->h_lay_n[k] = w_hi - w_lo + 1; }
        }
    }
    long long off = 0;
    for (int k = 0; k < G.gz; k++) {
        c->h_lay_off[k] = (int)off;
        off += (long long)c->h_lay_n[k] * c->h_lay_n[k];
    }
    if (off > 0x7fff0000LL) return amc_fail(c, AMC_ERR_INVALID, "detection grid too large (%lld cells)", off);
    G.ncells = (int)off;
    AMC_HIP(c, dalloc(c, &c->d_lay, (size_t)3 * G.gz));
    AMC_HIP(c, hipMemcpy(c->d_lay, c->h_lay_lo.data(), sizeof(int) * G.gz, hipMemcpyHostToDevice));
    AMC_HIP(c, hipMemcpy(c->d_lay + G.gz, c->h_lay_n.data(), sizeof(int) * G.gz, hipMemcpyHostToDevice));
    AMC_HIP(c, hipMemcpy(c->d_lay + 2 * G.gz, c->h_lay_off.data(), sizeof(int) * G.gz, hipMemcpyHostToDevice));
    G.lay_lo = c->d_lay; G.lay_n = c->d_lay + G.gz; G.lay_off = c->d_lay + 2 * G.gz;
    return AMC_OK;
}

// ---- amc_create in steps ---------------------------------------------------------------------------------------------------
// The environment switches, read once per context.  Three spellings, each switch keeps its own: set at all, set to a
// non-zero number, a number with a default.
static bool env_set(const char *name) { return getenv(name) != nullptr; }
static bool env_nonzero(const char *name) { const char *e = getenv(name); return e && atoi(e) != 0; }
static int env_int(const char *name, int unset) { const char *e = getenv(name); return e ? atoi(e) : unset; }
static long long env_ll(const char *name, long long unset) { const char *e = getenv(name); return e ? atoll(e) : unset; }

static void read_env(amc_ctx *c)
{
    const char *sync = getenv("AMC_OVERLAP_SYNC");
    c->ovl_sync_values = sync && !strcmp(sync, "value");
    // AMC_OVERLAP: 1 the streaming pass of step s + 1 runs beside the resolve of sweep s inside amc_run, on a second stream;
    // 2 the same kernels in order on one stream (debugging); 0 the plain sequence (the default: measured on MI355X the resolve
    // kernels take twice as long beside the pass's memory traffic, which with the fix-up kernel and the two cross-stream
    // dependencies of a step eats what the overlap hides — DESIGN 4.2 has the numbers)
    c->overlap_mode = env_int("AMC_OVERLAP", 0);
    c->overlap_split = env_nonzero("AMC_OVERLAP_SPLIT");                                 // (experiment)
    c->cw_blocks_env = env_int("AMC_CW_BLOCKS", 0);
    c->cw_dense_max = std::max(env_int("AMC_CW_DENSE_MAX", c->cw_dense_max), 0);        // (0: the list form always)
    c->ordered_always = env_nonzero("AMC_ORDERED_ALWAYS");
    c->od_max_n = env_ll("AMC_OD_MAX_N", c->od_max_n);                                   // (tests, experiments)
    c->od_ahead = std::min(std::max(env_int("AMC_OD_AHEAD", c->od_ahead), 1), 32);       // (experiments)
    if (const int v = env_int("AMC_PLAN_SMALL", -1); v >= 0) c->plan_small = v;
    c->stream_bs = env_int("AMC_STREAM_BS", 256);      // (experiments: 64 / 128 / 256)
    c->detect_bs = env_int("AMC_DETECT_BS", 256);      // (experiments: 64 / 128 / 256)
    c->temp_unfused = env_set("AMC_TEMP_UNFUSED");     // cross-check path: one hits/sample/apply triple per case
    // amc_temp_run_device: AMC_TEMP_RUN_UNFUSED=1 enqueues the single step's three streaming passes (the cross-check form),
    // AMC_TEMP_RUN_FUSED=1 the one fused pass; without either, what AMC_TEMP_RUN_FUSED_DEFAULT says
    c->temp_run_unfused = !AMC_TEMP_RUN_FUSED_DEFAULT;
    if (env_nonzero("AMC_TEMP_RUN_FUSED")) c->temp_run_unfused = false;
    if (env_nonzero("AMC_TEMP_RUN_UNFUSED")) c->temp_run_unfused = true;
    // AMC_ALLPAIRS_MAX_N restores a size threshold below which cube / pore contexts run without the grid (experiments)
    c->allpairs_max_n = env_ll("AMC_ALLPAIRS_MAX_N", 0);
    // kept lists (amc_lists): AMC_LIST_KEEP=K, a full build every K steps
    const int g = c->P.geometry;
    c->list_keep = env_int("AMC_LIST_KEEP", (g == AMC_GEOM_PORE || g == AMC_GEOM_PORE_ENERGISED) ? AMC_LIST_KEEP_DEFAULT_PORE : 0);
    // AMC_MAX_HIST (diagnostic): the history / overlay entries a sweep may USE (the allocation keeps its size): lets a test
    // drive the wide kernel's overlay protocol into its capacity limit at sizes the oracle handles in seconds
    c->max_hist_env = env_int("AMC_MAX_HIST", 0);
    c->debug_resolve = env_set("AMC_DEBUG_RESOLVE");
}

// the particle state in ONE allocation: the resolve kernels gather the eleven fields of a particle from eleven arrays — in
// one slab they share address-translation entries instead of needing one each
static int alloc_state(amc_ctx *c)
{
    const size_t n = std::max<size_t>((size_t)c->n, 1);
    double **st[] = {&c->S.x, &c->S.y, &c->S.z, &c->S.vx, &c->S.vy, &c->S.vz, &c->S.d, &c->S.dx, &c->S.dy, &c->S.dz,
                     &c->S.px, &c->S.py, &c->S.pz};
    const size_t per = ((sizeof(double) * n) + 255) & ~(size_t)255;
    const size_t total = 13 * per + ((n + 255) & ~(size_t)255);
    AMC_HIP(c, dalloc(c, &c->s_slab, total));
    AMC_HIP(c, hipMemsetAsync(c->s_slab, 0, total, c->stream));
    size_t off = 0;
    for (auto pp : st) { *pp = (double *)(c->s_slab + off); off += per; }
    c->S.flag = (uint8_t *)(c->s_slab + off);
    c->S_buf[0] = c->S;
    return AMC_OK;
}

// the detection grid and the per-cell lists over it (nothing without a grid)
static int alloc_grid_lists(amc_ctx *c)
{
    if (int rc = setup_grid(c)) return rc;
    if (c->allpairs) return AMC_OK;
    const size_t n = (size_t)c->n, nc = (size_t)c->G.ncells;
    c->max_extra = AMC_EXTRA_NODES(c->n);
    // kept lists: off in an overlapped run (its fix-up kernel files particles itself) and when the all-pairs detector is in
    // front.  (The energised pore files its particles in the bounds pass that follows the wall cases, amc_temp_end: the same
    // pass, the same cycle.)
    size_t pool = 0, keep_waves = 0;
    int K = c->list_keep;
    if (c->overlap_mode || c->detect_ap || c->P.geometry == AMC_GEOM_CELL) K = 0;
    const int threads = c->stream_bs;
    const long long nwaves = (((long long)n + threads - 1) / threads) * (threads / 64);
    // (a wave's pool holds everything its 64 particles could hand out in K - 1 steps; shorter cycles rather than more
    // than 2^30 nodes)
    while (K >= 2 && (long long)n + nwaves * 64 * (K - 1) > 0x3fffffffLL) K--;
    if (K >= 2 && n > 0 && threads % 64 == 0) {
        c->keep_K = K;
        c->B.wave_cap = 64 * (K - 1);
        pool = (size_t)c->B.wave_cap * (size_t)nwaves;
        keep_waves = (size_t)nwaves;
    }
    c->keep_pool = pool;
    AMC_HIP(c, dalloc(c, &c->B.rec, n + std::max((size_t)c->max_extra, pool)));
    AMC_HIP(c, dalloc(c, &c->B.head, nc + 1));
    AMC_HIP(c, hipMemsetAsync(c->B.head, 0, sizeof(unsigned long long) * (nc + 1), c->stream));
    c->B.n = (int)c->n;
    if (c->keep_K >= 2) {
        AMC_HIP(c, dalloc(c, &c->B.extra, pool));
        AMC_HIP(c, dalloc(c, &c->B.cell_of, n));
        AMC_HIP(c, dalloc(c, &c->B.node_of, n));
        AMC_HIP(c, dalloc(c, &c->B.wave_count, keep_waves));
        AMC_HIP(c, hipMemsetAsync(c->B.wave_count, 0, sizeof(int) * keep_waves, c->stream));
    }
    c->B_buf[0] = c->B;
    AMC_HIP(c, dalloc(c, &c->W.ov_head, nc));
    AMC_HIP(c, hipMemsetAsync(c->W.ov_head, 0xff, sizeof(int) * std::max<size_t>(nc, 1), c->stream));
    return AMC_OK;
}

// ONE allocation for the whole sweep work space: the resolve kernels are chains of dependent, scattered accesses to some
// sixty small arrays — carved from one slab they share a handful of translation entries instead of one each
static int alloc_resolve_ws(amc_ctx *c)
{
    amc_resolve_ws &W = c->W;
    const size_t n = (size_t)c->n;
    long long mc = c->P.max_candidates > 0 ? c->P.max_candidates : std::max<long long>(4096, c->n / 8 + 1024);
    if (mc > 0x3fffffff) mc = 0x3fffffff;
    W.max_cand = (int)mc;
    // every candidate brings two slots of its own (2k, 2k + 1); particles that join a cluster later take theirs from a counter
    W.max_slots = (int)std::min<long long>(2 * mc + std::max<long long>(1024, mc / 2), 0x7ffffff0LL);
    W.max_edges = 4 * W.max_slots + 1024;
    W.max_hist = 8 * W.max_slots + 1024;
    const size_t ms = (size_t)W.max_slots;
    auto carve = [&](char *base) -> size_t {
        size_t off = 0;
        auto take = [&](auto **pp, size_t count) {
            using T = std::remove_pointer_t<std::remove_pointer_t<decltype(pp)>>;
            off = (off + 255) & ~(size_t)255;
            *pp = base ? (T *)(base + off) : nullptr;
            off += sizeof(T) * std::max<size_t>(count, 1);
        };
        take(&W.ctl, 64); take(&W.wctl, 64);
        take(&W.cand4, (size_t)W.max_cand); take(&W.cand_s, (size_t)W.max_cand); take(&W.cand_mark, (size_t)W.max_cand);
        take(&W.sl_meta, ms); take(&W.sl_hits, ms); take(&W.sl_moved, ms);
        take(&W.sl_state, (size_t)RS_SLOT_DOUBLES * ms);
        take(&W.sl_label, ms); take(&W.sl_tmp, ms); take(&W.sl_dirty, ms); take(&W.order, ms);
        take(&W.sl_key, (size_t)next_pow2(W.max_slots));
        for (int k = 0; k < 10; k++) take(&W.cw_d[k], ms);
        take(&W.cw_tmp, ms); take(&W.cw_pidx, ms); take(&W.cw_slot, ms); take(&W.cw_flag, ms); take(&W.cw_moved, ms);
        take(&W.edge_a, (size_t)W.max_edges); take(&W.edge_b, (size_t)W.max_edges);
        take(&W.hist, (size_t)W.max_hist); take(&W.ov_next, (size_t)W.max_hist);
        take(&W.ev_gen, (size_t)W.max_hist); take(&W.ev, (size_t)W.max_hist);
        take(&W.adj_head, n); take(&W.slot_of, n); take(&W.victim, n);
        return (off + 255) & ~(size_t)255;
    };
    const size_t total = carve(nullptr);
    AMC_HIP(c, dalloc(c, &c->w_slab, total));
    AMC_HIP(c, hipMemsetAsync(c->w_slab, 0, total, c->stream));
    carve(c->w_slab);
    if (c->max_hist_env > 0 && c->max_hist_env < W.max_hist) W.max_hist = c->max_hist_env;
    amc_resolve_ctl z;
    memset(&z, 0, sizeof z);
    z.cur_round = 1;
    AMC_HIP(c, hipMemcpyAsync(W.wctl, &z, sizeof z, hipMemcpyHostToDevice, c->stream));
    AMC_HIP(c, hipStreamSynchronize(c->stream));
    AMC_HIP(c, hipMemsetAsync(W.slot_of, 0xff, sizeof(int) * std::max<size_t>(n, 1), c->stream));
    return AMC_OK;
}

// path records, counters and their banks, histograms
static int alloc_outputs(amc_ctx *c)
{
    const amc_params *p = &c->P;
    long long mp = p->max_paths > 0 ? p->max_paths : (p->max_paths < 0 ? 0 : (1LL << 20));   // < 0: histograms only
    if (mp > 0x7fffffff) mp = 0x7fffffff;
    if (mp > 0) AMC_HIP(c, dalloc(c, &c->d_rec, (size_t)mp));
    AMC_HIP(c, dalloc(c, &c->d_cnt, 1));
    AMC_HIP(c, hipMemsetAsync(c->d_cnt, 0, sizeof(amc_dev_counters), c->stream));
    AMC_HIP(c, dalloc(c, &c->d_banks, AMC_COUNTER_BANKS));
    AMC_HIP(c, hipMemsetAsync(c->d_banks, 0, sizeof(amc_counter_bank) * AMC_COUNTER_BANKS, c->stream));
    c->out.banks = c->d_banks;
    c->out.rec = c->d_rec; c->out.cap = (unsigned)mp; c->out.cnt = c->d_cnt;
    c->out.lo = p->hist_lo; c->out.hi = p->hist_hi;
    if (p->hist_bins > 0 && p->hist_hi > p->hist_lo) {
        const int nb = p->hist_bins;
        AMC_HIP(c, dalloc(c, &c->d_hist, (size_t)4 * nb * AMC_COUNTER_BANKS));
        AMC_HIP(c, hipMemsetAsync(c->d_hist, 0, sizeof(unsigned long long) * 4 * nb * AMC_COUNTER_BANKS, c->stream));
        AMC_HIP(c, dalloc(c, &c->d_edges, (size_t)nb + 1));
        // np.linspace(lo, hi, nb+1): start + k*step with step = (hi-lo)/nb, last element forced to hi
        std::vector<double> ed(nb + 1);
        const double step = (p->hist_hi - p->hist_lo) / (double)nb;
        for (int k = 0; k <= nb; k++) ed[k] = p->hist_lo + (double)k * step;
        ed[nb] = p->hist_hi;
        AMC_HIP(c, hipMemcpy(c->d_edges, ed.data(), sizeof(double) * (nb + 1), hipMemcpyHostToDevice));
        c->out.nbins = nb; c->out.hist = c->d_hist; c->out.edges = c->d_edges; c->out.bin_step = step;
    }
    return AMC_OK;
}

// the host-mapped words of the launch plans, the on-demand run's device words, the pinned staging buffer
static int alloc_host_words(amc_ctx *c)
{
    void *hp = nullptr, *dp = nullptr;
    // (three words, a cache line apart: candidate count; mirror of stalled_at; last step whose wide kernel ran)
    if (palloc(c, &hp, 256, hipHostMallocMapped) == hipSuccess && hipHostGetDevicePointer(&dp, hp, 0) == hipSuccess) {
        memset(hp, 0, 256);
        c->h_host_ncand = (volatile int *)hp;
        c->d_host_ncand = (int *)dp;
        c->h_od_stall = (volatile int *)hp + 16; c->d_od_stall_host = (int *)dp + 16;
        c->h_od_done = (volatile int *)hp + 32; c->d_od_done_host = (int *)dp + 32;
    }
    AMC_HIP(c, dalloc(c, &c->d_od, 16));
    AMC_HIP(c, hipMemsetAsync(c->d_od, 0, 16 * sizeof(int), c->stream));
    if (palloc(c, &c->h_pin, (size_t)4 << 20, hipHostMallocDefault) == hipSuccess) c->h_pin_bytes = (size_t)4 << 20;
    return AMC_OK;
}

extern "C" {

int amc_abi_version(void) { return AMC_ABI_VERSION; }

const char *amc_last_error(const amc_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

const char *amc_kernel_name(int k)
{
    static const char *names[AMC_K_COUNT] = {"drift_walls", "bin_count", "bin_scan",     "bin_scatter", "detect",  "resolve",
                                             "bounds",      "validate",  "resolve_more", "commit",      "clusters_wide", "fixup",
                                             "fields"};
    return (k >= 0 && k < AMC_K_COUNT) ? names[k] : "?";
}

void amc_destroy(amc_ctx *c)
{
    if (!c) return;
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);
    ctx_free_since(c, 0);
    delete c;
}

int amc_create(amc_ctx **out, const amc_params *p)
{
    if (!out || !p) { g_create_err = "null argument"; return AMC_ERR_INVALID; }
    *out = nullptr;
    if (p->struct_size != (int32_t)sizeof(amc_params)) {
        g_create_err = "amc_params.struct_size mismatch (ABI)";
        return AMC_ERR_INVALID;
    }
    if (p->n < 0 || p->n > 0x7fffffffLL || !(p->collision_range > 0) || !(p->argon_mass > 0) || p->geometry < 0 ||
        p->geometry > AMC_GEOM_PORE_ENERGISED) {
        g_create_err = "invalid amc_params (n, collision_range, argon_mass or geometry)";
        return AMC_ERR_INVALID;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || p->device < 0 || p->device >= ndev) {
        g_create_err = "no usable HIP device (libargonmc has no CPU fallback)";
        return AMC_ERR_NO_DEVICE;
    }
    amc_ctx *c = new (std::nothrow) amc_ctx();
    if (!c) { g_create_err = "out of host memory"; return AMC_ERR_INVALID; }
    c->P = *p;
    c->device = p->device;
    c->n = p->n; c->hi = p->n;
    c->keep_prior = (p->reserved0 & 1) != 0;
    read_env(c);
    // a failure below returns through amc_fail: the guard hands its message on and destroys what was built
    std::unique_ptr<amc_ctx, void (*)(amc_ctx *)> guard(c, [](amc_ctx *x) { g_create_err = x->err; amc_destroy(x); });
    AMC_HIP(c, hipSetDevice(c->device));
    AMC_HIP(c, ctx_stream(c, &c->own_stream));
    c->stream = c->own_stream;
    // detection mode: only single cells (AMC_GEOM_CELL: no geometry to lay a grid over) run without the detection grid —
    // all-pairs detector, brute-force validation, everything in the one ordered workgroup.  Cube and pore contexts use
    // the grid and the wide cluster kernel at ANY size: measured at N = 4,096 the grid path takes 32 us per step, the
    // gridless one 132 (N = 1,000: 28 against 45; round 2 sent N <= 4,096 down the gridless path).
    // (detect_mode 2: the all-pairs DETECTOR in front of the same grid-based resolve — the kernel the reference's
    // pairwise loop maps to directly, measurable at full size against the fp64 vector peak)
    c->allpairs = (p->geometry == AMC_GEOM_CELL) || (p->detect_mode != 1 && c->n <= c->allpairs_max_n);
    c->detect_ap = c->allpairs || p->detect_mode == 2;
    if (p->geometry == AMC_GEOM_CELL && p->detect_mode == 1) {
        return amc_fail(c, AMC_ERR_INVALID, "AMC_GEOM_CELL has no cell grid: detect_mode must be 0 or 2");
    }
    int rc;
    if ((rc = alloc_state(c)) || (rc = alloc_grid_lists(c)) || (rc = alloc_resolve_ws(c)) || (rc = alloc_outputs(c)) ||
        (rc = alloc_host_words(c)))
        return rc;
    if (c->debug_resolve) {
        AMC_HIP(c, dalloc(c, &c->d_dbg, 128 + 128 * 512));
        AMC_HIP(c, hipMemsetAsync(c->d_dbg, 0, sizeof(long long) * (128 + 128 * 512), c->stream));
        { const long long big = 0x7fffffffffffffffLL; AMC_HIP(c, hipMemcpyAsync(c->d_dbg + 28, &big, sizeof big, hipMemcpyHostToDevice, c->stream)); }
    }
    AMC_HIP(c, hipStreamSynchronize(c->stream));
    *out = guard.release();
    return AMC_OK;
}

int amc_set_stream(amc_ctx *c, void *hip_stream)
{
    if (!c) return AMC_ERR_INVALID;
    hipSetDevice(c->device);
    amc_prof_collect(c);
    if (c->stream) hipStreamSynchronize(c->stream);
    c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
    return AMC_OK;
}

int amc_use_null_stream(amc_ctx *c)
{
    if (!c) return AMC_ERR_INVALID;
    hipSetDevice(c->device);
    amc_prof_collect(c);
    if (c->stream) hipStreamSynchronize(c->stream);
    c->stream = nullptr;        // HIP's NULL stream
    return AMC_OK;
}

int amc_synchronize(amc_ctx *c)
{
    if (!c) return AMC_ERR_INVALID;
    AMC_HIP(c, hipSetDevice(c->device));
    AMC_HIP(c, hipStreamSynchronize(c->stream));
    return AMC_OK;
}

int amc_upload(amc_ctx *c, const double *x, const double *y, const double *z, const double *vx, const double *vy,
               const double *vz, const double *dist, const double *dist_x, const double *dist_y, const double *dist_z,
               const uint8_t *full_path)
{
    if (!c) return AMC_ERR_INVALID;
    AMC_HIP(c, hipSetDevice(c->device));
    { int rc_ = amc_flush(c); if (rc_) return rc_; }
    c->step.lists_age = -1;          // (kept lists: a new state starts with a full build)
    amc_mg_step_fresh(c);            // (and a pending pack describes the old one)
    const size_t nb = sizeof(double) * (size_t)c->n;
    const double *src[] = {x, y, z, vx, vy, vz, dist, dist_x, dist_y, dist_z};
    double *dst[] = {c->S.x, c->S.y, c->S.z, c->S.vx, c->S.vy, c->S.vz, c->S.d, c->S.dx, c->S.dy, c->S.dz};
    for (int k = 0; k < 10; k++)
        if (src[k] && nb) AMC_HIP(c, hipMemcpyAsync(dst[k], src[k], nb, hipMemcpyHostToDevice, c->stream));
    if (full_path && c->n) AMC_HIP(c, hipMemcpyAsync(c->S.flag, full_path, (size_t)c->n, hipMemcpyHostToDevice, c->stream));
    { int rc_ = amc_publish_velocities(c); if (rc_) return rc_; }
    AMC_HIP(c, hipStreamSynchronize(c->stream));
    c->uploaded = true;
    return AMC_OK;
}

int amc_publish_velocities(amc_ctx *c)
{
    if (!c->MG.kin_vpub || c->n <= 0) return AMC_OK;       // not a sharded context
    const size_t nb = sizeof(double) * (size_t)c->n;
    const double *src[3] = {c->S.vx, c->S.vy, c->S.vz};
    for (int e = 0; e < 3; e++)
        AMC_HIP(c, hipMemcpyAsync(c->MG.kin_vpub + (size_t)e * (size_t)c->n, src[e], nb, hipMemcpyDeviceToDevice, c->stream));
    return AMC_OK;
}

int amc_download(amc_ctx *c, double *x, double *y, double *z, double *vx, double *vy, double *vz, double *dist,
                 double *dist_x, double *dist_y, double *dist_z, uint8_t *full_path)
{
    if (!c) return AMC_ERR_INVALID;
    AMC_HIP(c, hipSetDevice(c->device));
    { int rc_ = amc_flush(c); if (rc_) return rc_; }
    const size_t nb = sizeof(double) * (size_t)c->n;
    double *dst[] = {x, y, z, vx, vy, vz, dist, dist_x, dist_y, dist_z};
    double *src[] = {c->S.x, c->S.y, c->S.z, c->S.vx, c->S.vy, c->S.vz, c->S.d, c->S.dx, c->S.dy, c->S.dz};
    for (int k = 0; k < 10; k++)
        if (dst[k] && nb) AMC_HIP(c, hipMemcpyAsync(dst[k], src[k], nb, hipMemcpyDeviceToHost, c->stream));
    if (full_path && c->n) AMC_HIP(c, hipMemcpyAsync(full_path, c->S.flag, (size_t)c->n, hipMemcpyDeviceToHost, c->stream));
    AMC_HIP(c, hipStreamSynchronize(c->stream));
    return AMC_OK;
}

int amc_download_prior(amc_ctx *c, double *px, double *py, double *pz)
{
    if (!c) return AMC_ERR_INVALID;
    if (!c->keep_prior) return amc_fail(c, AMC_ERR_STATE, "prior_*_vals are only kept when amc_params.reserved0 bit0 is set");
    AMC_HIP(c, hipSetDevice(c->device));
    const size_t nb = sizeof(double) * (size_t)c->n;
    if (px && nb) AMC_HIP(c, hipMemcpyAsync(px, c->S.px, nb, hipMemcpyDeviceToHost, c->stream));
    if (py && nb) AMC_HIP(c, hipMemcpyAsync(py, c->S.py, nb, hipMemcpyDeviceToHost, c->stream));
    if (pz && nb) AMC_HIP(c, hipMemcpyAsync(pz, c->S.pz, nb, hipMemcpyDeviceToHost, c->stream));
    AMC_HIP(c, hipStreamSynchronize(c->stream));
    return AMC_OK;
}

// ---- outputs ----------------------------------------------------------------------------------------------------------
int amc_paths_pending(amc_ctx *c, size_t *n)
{
    if (!c || !n) return AMC_ERR_INVALID;
    AMC_HIP(c, hipSetDevice(c->device));
    amc_dev_counters now;
    int rc = amc_read_counters(c, &now);
    if (rc) return rc;
    *n = std::min<size_t>(now.path_count, c->out.cap);
    return AMC_OK;
}

int amc_drain_paths(amc_ctx *c, amc_path_record *out, size_t cap, size_t *n)
{
    if (!c || !n) return AMC_ERR_INVALID;
    size_t pending;
    int rc = amc_paths_pending(c, &pending);
    if (rc) return rc;
    if (pending > cap) return amc_fail(c, AMC_ERR_CAPACITY, "amc_drain_paths: %zu records pending, buffer holds %zu", pending, cap);
    if (pending) AMC_HIP(c, hipMemcpyAsync(out, c->d_rec, sizeof(amc_path_record) * pending, hipMemcpyDeviceToHost, c->stream));
    unsigned int zero = 0;
    AMC_HIP(c, hipMemcpyAsync(&c->d_cnt->path_count, &zero, sizeof zero, hipMemcpyHostToDevice, c->stream));
    if (c->MF.on) { int rc_ = amc_mfp_rewind(c); if (rc_) return rc_; }     // (the sampled free paths' cursor with it)
    AMC_HIP(c, hipStreamSynchronize(c->stream));
    *n = pending;
    return AMC_OK;
}

int amc_histograms(amc_ctx *c, uint64_t *counts, uint64_t *n_paths_total)
{
    if (!c) return AMC_ERR_INVALID;
    AMC_HIP(c, hipSetDevice(c->device));
    if (counts) {
        if (!c->d_hist) return amc_fail(c, AMC_ERR_STATE, "histograms disabled (hist_bins == 0)");
    }
    // the pending commit first: the bins copied below and the total read after them describe the same sweeps
    { int rc_ = amc_settle_commit(c); if (rc_) return rc_; }
    std::vector<uint64_t> banks;
    if (counts) {
        banks.resize((size_t)4 * c->out.nbins * AMC_COUNTER_BANKS);
        AMC_HIP(c, hipMemcpyAsync(banks.data(), c->d_hist, sizeof(uint64_t) * banks.size(), hipMemcpyDeviceToHost, c->stream));
    }
    amc_dev_counters now;
    int rc = amc_read_counters(c, &now);        // (synchronises the stream)
    if (rc) return rc;
    if (counts) {
        const size_t m = (size_t)4 * c->out.nbins;
        for (size_t k = 0; k < m; k++) counts[k] = 0;
        for (int b = 0; b < AMC_COUNTER_BANKS; b++)
            for (size_t k = 0; k < m; k++) counts[k] += banks[(size_t)b * m + k];
    }
    if (n_paths_total) *n_paths_total = now.n_paths_total;
    return AMC_OK;
}

int amc_reset_outputs(amc_ctx *c)
{
    if (!c) return AMC_ERR_INVALID;
    AMC_HIP(c, hipSetDevice(c->device));
    // a commit still pending runs now, so that what it emits is discarded with the rest instead of landing in the zeroed
    // outputs with the next streaming pass; the sweep's deferred results stay in the slot arrays (step.lazy_pending) and
    // reach the particle arrays as they would have
    { int rc_ = amc_settle_commit(c); if (rc_) return rc_; }
    if (c->d_hist) AMC_HIP(c, hipMemsetAsync(c->d_hist, 0, sizeof(uint64_t) * 4 * c->out.nbins * AMC_COUNTER_BANKS, c->stream));
    AMC_HIP(c, hipMemsetAsync(c->d_cnt, 0, sizeof(amc_dev_counters), c->stream));
    AMC_HIP(c, hipMemsetAsync(c->d_banks, 0, sizeof(amc_counter_bank) * AMC_COUNTER_BANKS, c->stream));
    if (c->MF.on) { int rc_ = amc_mfp_rewind(c); if (rc_) return rc_; }     // (path_count is zero: the sampled free paths' cursor with it)
    AMC_HIP(c, hipStreamSynchronize(c->stream));
    memset(&c->h_prev, 0, sizeof c->h_prev);
    c->out.step = 0;
    return AMC_OK;
}

// ---- pairwise_particles_in_cell replacement ---------------------------------------------------------------------------
int amc_pairwise_cell(amc_ctx *c, int64_t n_cell, double *continue_path, double *continue_x_path, double *continue_y_path,
                      double *continue_z_path, uint8_t *has_collided, double *x, double *y, double *z, double *vx,
                      double *vy, double *vz, double *out_paths, size_t cap, size_t *n_paths, int64_t *n_collisions)
{
    if (!c) return AMC_ERR_INVALID;
    if (c->P.geometry != AMC_GEOM_CELL) return amc_fail(c, AMC_ERR_STATE, "amc_pairwise_cell needs an AMC_GEOM_CELL context");
    if (n_cell < 0 || n_cell > c->n) return amc_fail(c, AMC_ERR_INVALID, "n_cell %lld exceeds the context capacity %lld", (long long)n_cell, (long long)c->n);
    AMC_HIP(c, hipSetDevice(c->device));
    // the context is sized for its capacity; run on the first n_cell entries
    const int64_t n_full = c->n;
    c->n = n_cell; c->lo = 0; c->hi = n_cell;
    int rc = amc_upload(c, x, y, z, vx, vy, vz, continue_path, continue_x_path, continue_y_path, continue_z_path, has_collided);
    amc_step_stats st;
    memset(&st, 0, sizeof st);
    size_t pending = 0;
    if (!rc) {
        size_t dummy;
        rc = amc_paths_pending(c, &dummy);          // discard nothing: records of earlier calls were drained by them
    }
    if (!rc) rc = amc_timestep(c, 0.0, &st);
    if (!rc) rc = amc_download(c, x, y, z, vx, vy, vz, continue_path, continue_x_path, continue_y_path, continue_z_path, has_collided);
    if (!rc) rc = amc_paths_pending(c, &pending);
    if (!rc && pending) {
        std::vector<amc_path_record> rec(pending);
        size_t got = 0;
        rc = amc_drain_paths(c, rec.data(), pending, &got);
        if (!rc) {
            // the reference appends in loop order: i ascending, j ascending, particle j before particle i
            std::sort(rec.begin(), rec.begin() + got, [](const amc_path_record &a, const amc_path_record &b) {
                if (a.step != b.step) return a.step < b.step;
                if (a.i != b.i) return a.i < b.i;
                if (a.j != b.j) return a.j < b.j;
                return a.which < b.which;
            });
            if (got > cap) rc = amc_fail(c, AMC_ERR_CAPACITY, "out_paths holds %zu paths, %zu were completed", cap, got);
            else if (out_paths)
                for (size_t k = 0; k < got; k++) {
                    out_paths[0 * cap + k] = rec[k].total; out_paths[1 * cap + k] = rec[k].px;
                    out_paths[2 * cap + k] = rec[k].py; out_paths[3 * cap + k] = rec[k].pz;
                }
            pending = got;
        }
    }
    if (n_paths) *n_paths = pending;
    if (n_collisions) *n_collisions = st.n_pp;
    c->n = n_full; c->lo = 0; c->hi = n_full;
    return rc;
}

// ---- measurement ------------------------------------------------------------------------------------------------------
int amc_profile(amc_ctx *c, int enable)
{
    if (!c) return AMC_ERR_INVALID;
    hipSetDevice(c->device);
    amc_prof_collect(c);
    c->profiling = enable != 0;
    return AMC_OK;
}

int amc_overlap_stats(amc_ctx *c, int64_t *out)
{
    if (!c || !out) return AMC_ERR_INVALID;
    AMC_HIP(c, hipSetDevice(c->device));
    amc_dev_counters now;
    int rc = amc_read_counters(c, &now);
    if (rc) return rc;
    out[0] = c->ovl_steps; out[1] = now.n_refiled; out[2] = c->overlap_mode; out[3] = c->max_extra;
    out[4] = c->od_ordered_launches; out[5] = c->od_steps; out[6] = c->od_stalls; out[7] = c->od_stalls_last;
    return AMC_OK;
}

// The kept lists as they stand (amc_lists, amc_step_state): reads only — one synchronisation and one copy of the owner's wave
// counters, no kernel, nothing settled or flushed: whatever a step left pending stays pending.
int amc_lists_stats(amc_ctx *c, int64_t *out)
{
    if (!c || !out) return AMC_ERR_INVALID;
    AMC_HIP(c, hipSetDevice(c->device));
    const amc_step_state &T = c->step;
    const bool cycle = c->keep_K >= 2 && T.lists_age >= 0;
    const int owner = cycle ? T.lists_owner : 0;
    const int *counts = nullptr;
    size_t waves = 0;
    // (the counters are the last owner's, also once its cycle has ended: lists_owner outlives lists_age)
    if (c->keep_K >= 2 && T.lists_owner == 2 && c->MG.keep && c->MG.wave_count) {
        counts = c->MG.wave_count; waves = (size_t)c->MG.waves_pack + (size_t)c->MG.waves_unpack;
    } else if (c->keep_K >= 2 && c->B.wave_count) {
        // (the streaming pass's own waves, as alloc_grid_lists counted them: keep_pool may have grown for the exchange kernels)
        counts = c->B.wave_count; waves = (size_t)((c->n + c->stream_bs - 1) / c->stream_bs) * (size_t)(c->stream_bs / 64);
    }
    int64_t sum = 0, top = 0;
    AMC_HIP(c, hipStreamSynchronize(c->stream));
    if (counts && waves) {
        std::vector<int> h(waves);
        AMC_HIP(c, hipMemcpy(h.data(), counts, sizeof(int) * waves, hipMemcpyDeviceToHost));
        for (int v : h) { sum += v; top = std::max<int64_t>(top, v); }
    }
    out[0] = c->keep_K >= 2 ? c->keep_K : 0; out[1] = c->keep_K >= 2 ? c->B.wave_cap : 0; out[2] = (int64_t)waves;
    out[3] = cycle ? T.lists_age : -1; out[4] = owner; out[5] = sum; out[6] = top; out[7] = T.full_builds;
    return AMC_OK;
}

// What the context owns right now (amc_ctx::owned, amc_host.h): a host value, nothing is synchronised or launched.
int amc_owned_count(amc_ctx *c, int64_t *count)
{
    if (!c || !count) return AMC_ERR_INVALID;
    *count = (int64_t)c->owned.size();
    return AMC_OK;
}

int amc_kernel_times(amc_ctx *c, double *total_ms, int64_t *launches)
{
    if (!c) return AMC_ERR_INVALID;
    hipSetDevice(c->device);
    amc_prof_collect(c);
    if (c->d_dbg) {
        long long h[128];
        hipMemcpy(h, c->d_dbg, sizeof h, hipMemcpyDeviceToHost);
        const double n = h[11] > 0 ? (double)h[11] : 1.0;
        fprintf(stderr, "[amc k_resolve phases, us/launch] count-left %.1f claim %.1f | rounds: collect %.1f pairs %.1f clusters>=3: sort+load %.1f emulate %.1f | overlay %.1f validate %.1f commit %.1f | rounds %.2f cand %.1f complex-members %.2f launches %lld (idle hand-over only %lld) | body: labels in the work space %lld moved there %lld layers in LDS %lld rounds split %lld heads shared %lld sorted %lld pool global %lld sort global %lld later %lld clusters by a wave %lld by one lane %lld most complex members %lld dense sweeps linked %lld\n",
                h[0] / n / 100.0, h[1] / n / 100.0, h[6] / n / 100.0, h[7] / n / 100.0, h[2] / n / 100.0, h[3] / n / 100.0, h[14] / n / 100.0, h[4] / n / 100.0, h[5] / n / 100.0,
                h[8] / n, h[9] / n, h[10] / n, h[11], h[12], h[32], h[33], h[34], h[35], h[36], h[37], h[38], h[39], h[40], h[41], h[42], h[43], h[44]);
        fprintf(stderr, "[amc host candidate count] %d (what the next launch plan is chosen from)\n", c->h_host_ncand ? (int)*c->h_host_ncand : -1);
        if (h[12] > 0)
            fprintf(stderr, "[amc k_resolve idle hand-over, us/launch] entry -> counts read %.2f, -> hand-over written %.2f, -> through the barrier %.2f (%lld launches)\n",
                    h[16] / (double)h[12] / 100.0, h[17] / (double)h[12] / 100.0, h[18] / (double)h[12] / 100.0, h[12]);
        {
            // the wide kernel's waves keep their figures in 64 words each (amc_clusters.hip)
            std::vector<long long> wv((size_t)128 * 512);
            hipMemcpy(wv.data(), c->d_dbg + 128, sizeof(long long) * wv.size(), hipMemcpyDeviceToHost);
            long long s[128] = {0}, longest = 0;
            for (int w = 0; w < 512; w++) {
                for (int e = 3; e < 128; e++) if (e != 4) s[e] += wv[(size_t)128 * w + e];
                longest = std::max(longest, wv[(size_t)128 * w + 4]);
            }
            const double nl = h[25] > 0 ? (double)h[25] : 1.0;
            static const char *cn[8] = {"pair", "3-cluster", "4+-cluster", "not owner", "pair+again", "3-cluster+again", "4+-cluster+again", "not owner+again"};
            static const char *pn[12] = {"graph", "walk", "reserve", "small: after emulate", "pair emulate | by the wave: emulate", "publish", "grid probe", "first hop", "particles", "set-up", "overlay probe", "small: prepare"};
            fprintf(stderr, "[amc k_clusters_wide] working waves %lld in %lld launches; launch span (first working wave in -> last out) %.2f us, last out -> ordered workgroup in %.2f us, longest wave ever %.2f us; dense scans %lld\n",
                    s[3], h[25], h[27] / nl / 100.0, h[26] / nl / 100.0, longest / 100.0, s[125]);
            fprintf(stderr, "[three-particle path of lane 0] %lld times, %lld continued from the pair's hit; loads + slots %.2f us, emulation %.2f us\n", s[5], s[6],
                    s[7] / (double)std::max<long long>(1, s[5]) / 100.0, s[124] / (double)std::max<long long>(1, s[5]) / 100.0);
            fprintf(stderr, "[pair-wave lifetimes, 2.5 us buckets]");
            for (int k = 0; k < 8; k++) fprintf(stderr, " %lld", s[24 + k]);
            fprintf(stderr, "\n");
            for (int k = 0; k < 8; k++) {
                if (!s[16 + k]) continue;
                fprintf(stderr, "[amc k_clusters_wide %-16s %7lld waves, %5.1f us]", cn[k], s[16 + k], s[8 + k] / (double)s[16 + k] / 100.0);
                for (int e = 0; e < 12; e++) fprintf(stderr, " %s %.2f", pn[e], s[32 + 12 * k + e] / (double)s[16 + k] / 100.0);
                fprintf(stderr, "\n");
            }
        }
    }
    for (int k = 0; k < AMC_K_COUNT; k++) {
        if (total_ms) total_ms[k] = c->k_ms[k];
        if (launches) launches[k] = c->k_launches[k];
    }
    return AMC_OK;
}

}  // extern "C"
