// amc_host.h — host-side helpers shared by the C ABI translation units (amc_api*.hip, amc_run.hip): device allocation, the
// pinned staging of small read-backs, counters / per-step statistics, the deferred commit and the sweep driver.
#pragma once
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <new>

#include "amc_internal.h"

// ---- what a context owns ------------------------------------------------------------------------------------------------
// Every device and pinned allocation, stream and event of a context is made by dalloc / palloc / ctx_stream / ctx_event and
// recorded in amc_ctx::owned: ctx_free releases recorded objects (a buffer that is replaced), amc_destroy whatever is left.
static hipError_t ctx_record(amc_ctx *c, hipError_t e, void **p, amc_res_kind kind)
{
    if (e == hipSuccess) c->owned.push_back({*p, kind});
    else *p = nullptr;
    return e;
}
template <class T>
static hipError_t dalloc(amc_ctx *c, T **p, size_t count)       // device memory for count (at least one) elements
{ return ctx_record(c, hipMalloc((void **)p, sizeof(T) * std::max<size_t>(count, 1)), (void **)p, AMC_RES_DEVICE); }
template <class T>
static hipError_t palloc(amc_ctx *c, T **p, size_t bytes, unsigned int flags)     // pinned host memory
{ return ctx_record(c, hipHostMalloc((void **)p, bytes, flags), (void **)p, AMC_RES_PINNED); }
static hipError_t ctx_stream(amc_ctx *c, hipStream_t *s)
{ return ctx_record(c, hipStreamCreateWithFlags(s, hipStreamNonBlocking), (void **)s, AMC_RES_STREAM); }
static hipError_t ctx_event(amc_ctx *c, hipEvent_t *ev, unsigned int flags)
{ return ctx_record(c, hipEventCreateWithFlags(ev, flags), (void **)ev, AMC_RES_EVENT); }

static void ctx_release(const amc_res &r)
{
    if (r.kind == AMC_RES_DEVICE) (void)hipFree(r.p);
    else if (r.kind == AMC_RES_PINNED) (void)hipHostFree(r.p);
    else if (r.kind == AMC_RES_STREAM) (void)hipStreamDestroy((hipStream_t)r.p);
    else (void)hipEventDestroy((hipEvent_t)r.p);
}
template <class... P>
static void ctx_free(amc_ctx *c, P... ps)                       // (nullptr: nothing)
{
    for (const void *q : {(const void *)ps...})
        for (size_t k = c->owned.size(); q && k-- > 0;)
            if (c->owned[k].p == q) { ctx_release(c->owned[k]); c->owned.erase(c->owned.begin() + k); break; }
}
static void ctx_free_since(amc_ctx *c, size_t mark)             // all but the first `mark` objects, newest first
{
    for (; c->owned.size() > mark; c->owned.pop_back()) ctx_release(c->owned.back());
}

// All-or-nothing set-up of a lazily built work space: what is allocated while the group is open is released again when it
// goes out of scope (an early return on a failed call), unless keep() was called.  The caller builds into locals, calls
// keep() once everything succeeded, then publishes the pointers, its guard last.  Nothing older is freed while it is open.
struct amc_alloc_group {
    amc_ctx *c;
    size_t mark;
    explicit amc_alloc_group(amc_ctx *ctx) : c(ctx), mark(ctx->owned.size()) {}
    ~amc_alloc_group() { if (c) ctx_free_since(c, mark); }
    void keep() { c = nullptr; }
};

// Small device -> host read-backs go through the pinned staging buffer: queue any number of pieces, synchronise once,
// then copy out.  (Falls back to direct copies when a piece does not fit.)
struct amc_stage {
    amc_ctx *c;
    size_t off = 0;
    struct piece { void *dst; size_t off, bytes; };
    std::vector<piece> pieces;
    explicit amc_stage(amc_ctx *ctx) : c(ctx) {}
    hipError_t get(void *dst, const void *src, size_t bytes)
    {
        if (!bytes) return hipSuccess;
        const size_t at = (off + 63) & ~(size_t)63;
        if (!c->h_pin || at + bytes > c->h_pin_bytes) return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream);
        pieces.push_back({dst, at, bytes});
        off = at + bytes;
        return hipMemcpyAsync(c->h_pin + at, src, bytes, hipMemcpyDeviceToHost, c->stream);
    }
    hipError_t finish()
    {
        const hipError_t e = hipStreamSynchronize(c->stream);
        if (e == hipSuccess)
            for (auto &p : pieces) memcpy(p.dst, c->h_pin + p.off, p.bytes);
        pieces.clear();
        off = 0;
        return e;
    }
};

// (defined inside the extern "C" block of amc_run.hip — amc_publish_velocities: amc_api.hip; internal to the library, not part of the ABI)
#define AMC_INTERNAL extern "C" __attribute__((visibility("hidden")))
AMC_INTERNAL int amc_settle_commit(amc_ctx *c);                         // run the last sweep's commit if it is still pending (no synchronisation)
AMC_INTERNAL int amc_read_counters(amc_ctx *c, amc_dev_counters *h);    // device counters with the banks folded in (synchronises)
AMC_INTERNAL int amc_finish_stats(amc_ctx *c, amc_step_stats *out);     // per-step deltas + error flags
AMC_INTERNAL int amc_publish_velocities(amc_ctx *c);                    // multi-GPU: vpub = current velocities (after an upload)
AMC_INTERNAL int amc_flush(amc_ctx *c);                                 // write deferred sweep results to the particle arrays
AMC_INTERNAL int amc_enqueue_sweep(amc_ctx *c, bool counted = false, bool defer_commit = false);   // bin (unless counted) + detect + resolve
// what the cadence hook calls for a sampler whose sample is due (AMC_SAMPLERS below): one sample of the current state, enqueued
AMC_INTERNAL int amc_fields_enqueue(amc_ctx *c);                      // amc_fields.hip
AMC_INTERNAL int amc_corr_step(amc_ctx *c);                           // amc_corr.hip: at the window position, which it advances
AMC_INTERNAL int amc_flux_enqueue(amc_ctx *c);                        // amc_fields.hip
AMC_INTERNAL int amc_mfp_step(amc_ctx *c);                            // amc_mfp.hip: the step's path records; every completed step
AMC_INTERNAL int amc_vdf_enqueue(amc_ctx *c);                         // amc_vdf.hip
AMC_INTERNAL int amc_transit_enqueue(amc_ctx *c);                     // amc_transit.hip
AMC_INTERNAL int amc_pair_enqueue(amc_ctx *c);                        // amc_pair.hip
AMC_INTERNAL int amc_mfp_rewind(amc_ctx *c);                          // the record buffer has been emptied: the cursor follows (no synchronisation)

// amc_timestep, amc_run and the stage calls: not in the middle of a sharded step (the rule above amc_mg_step)
static inline int amc_mg_step_idle(amc_ctx *c, const char *who)
{
    if (c->MG.step.phase == AMC_MG_IDLE) return AMC_OK;
    return amc_fail(c, AMC_ERR_STATE, "%s in the middle of a sharded step (amc_mg_pack ... amc_mg_finish): finish it, or start over with "
                                      "amc_mg_local / amc_upload", who);
}

// ---- what the samplers share on the host (every amc_<sampler>.hip, the step drivers) ---------------------------------------------------------
// a sample is due after the step that leaves the step counter at `step`
static inline bool amc_cadence_due(bool on, int64_t every, int64_t step_offset, int64_t step) { return on && every > 0 && (step + step_offset) % every == 0; }

// The samplers of the particle state, ONE entry each, in the order the hook runs them.  A new sampler is one more line here:
// everything below is derived from the table.  cadence: the workspace's on, every and step_offset as they stand; step: what the hook
// calls when a sample is due.
#define AMC_EVERY_STEP (-1)     // amc_cadence::every of a sampler that is due after every step while it is on
struct amc_cadence { bool on; int64_t every, step_offset; };
struct amc_sampler { amc_cadence (*cadence)(const amc_ctx *c); int (*step)(amc_ctx *c); };
template <class WS>
static inline amc_cadence amc_cadence_of(const WS &W) { return amc_cadence{W.on, W.g.every, W.g.step_offset}; }
static const amc_sampler AMC_SAMPLERS[] = {
    {[](const amc_ctx *c) { return amc_cadence_of(c->F); }, amc_fields_enqueue},
    {[](const amc_ctx *c) { return amc_cadence_of(c->CR); }, amc_corr_step},
    {[](const amc_ctx *c) { return amc_cadence_of(c->FX); }, amc_flux_enqueue},
    // (the sampled free paths bin by the owner's position at the end of the step)
    {[](const amc_ctx *c) { return amc_cadence{c->MF.on, AMC_EVERY_STEP, 0}; }, amc_mfp_step},
    {[](const amc_ctx *c) { return amc_cadence_of(c->VD); }, amc_vdf_enqueue},
    {[](const amc_ctx *c) { return amc_cadence_of(c->TR); }, amc_transit_enqueue},
    {[](const amc_ctx *c) { return amc_cadence_of(c->PD); }, amc_pair_enqueue},
};
static inline bool amc_sampler_due(const amc_cadence &k, int64_t step)
{
    return k.every == AMC_EVERY_STEP ? k.on : amc_cadence_due(k.on, k.every, k.step_offset, step);
}
// a sampler is configured, with a cadence or without (every == 0: manual samples)
static inline bool amc_samplers_configured(const amc_ctx *c)
{
    for (const amc_sampler &s : AMC_SAMPLERS)
        if (s.cadence(c).on) return true;
    return false;
}
// a sample of some sampler is due after `step`: such a step ends with the state everybody reads (no deferred bounds pass)
static inline bool amc_samplers_due(const amc_ctx *c, int64_t step)
{
    for (const amc_sampler &s : AMC_SAMPLERS)
        if (amc_sampler_due(s.cadence(c), step)) return true;
    return false;
}
// a sampler runs on a cadence (some step is due): amc_run takes its plain loop
static inline bool amc_samplers_cadence(const amc_ctx *c)
{
    for (const amc_sampler &s : AMC_SAMPLERS) {
        const amc_cadence k = s.cadence(c);
        if (k.on && k.every != 0) return true;
    }
    return false;
}
// the cadence hook after a completed step
static inline int amc_samplers_step(amc_ctx *c)
{
    for (const amc_sampler &s : AMC_SAMPLERS)
        if (amc_sampler_due(s.cadence(c), (int64_t)c->out.step))
            if (int rc = s.step(c)) return rc;
    return AMC_OK;
}

// The checks the samplers' entry points start with; `name`: the entry points' prefix ("amc_vdf").  c is not null: they have looked.
// ... on a configured sampler (`what`: the entry point's name behind the prefix)
static inline int amc_sampler_ready(amc_ctx *c, bool on, const char *name, const char *what)
{
    if (!on) return amc_fail(c, AMC_ERR_STATE, "%s_%s before %s_config", name, what, name);
    AMC_HIP(c, hipSetDevice(c->device));
    return AMC_OK;
}
// ... amc_<s>_sample: configured, a state uploaded
static inline int amc_sampler_sample_ready(amc_ctx *c, bool on, const char *name)
{
    if (!on) return amc_fail(c, AMC_ERR_STATE, "%s_sample before %s_config", name, name);
    if (!c->uploaded) return amc_fail(c, AMC_ERR_STATE, "%s_sample before amc_upload", name);
    AMC_HIP(c, hipSetDevice(c->device));
    return AMC_OK;
}
// ... amc_<s>_config, up to the struct's own fields: a null grid switches the sampler off (free_ws(c) gives its buffers back,
// *done = true: the caller returns).  needs: what the sampler asks of the context, checked in front of the struct, or nullptr
template <class Grid, class Free>
static inline int amc_sampler_config_begin(amc_ctx *c, const Grid *g, const char *grid_name, Free free_ws, bool *done,
                                           int (*needs)(amc_ctx *c) = nullptr)
{
    *done = false;
    if (!c) return AMC_ERR_INVALID;
    AMC_HIP(c, hipSetDevice(c->device));
    AMC_HIP(c, hipStreamSynchronize(c->stream));        // (a sample or launch in flight may still use the old buffers)
    if (!g) {
        free_ws(c);
        *done = true;
        return AMC_OK;
    }
    if (needs)
        if (int rc = needs(c)) return rc;
    if (g->struct_size != (int32_t)sizeof(Grid)) return amc_fail(c, AMC_ERR_INVALID, "%s.struct_size mismatch (ABI)", grid_name);
    return AMC_OK;
}

// The grid fields amc_field_grid, amc_corr_grid, amc_flux_grid, amc_mfp_grid, amc_vdf_grid and amc_pair_grid have in common, validated (`who`: the struct's name, `unit`: what it calls its
// bins; reserved0: its reserved fields are zero; own_fault: a fault in the struct's other fields, reported at its place in the
// order, behind the bin count, or nullptr) and turned into the grid the kernels take, widths included.
static inline int amc_sample_grid_check(amc_ctx *c, const char *who, const char *unit, int kind, int n1, int n2, int n3, int max_bins,
                                 const double *lo, const double *hi, int64_t every, int64_t step_offset, bool reserved0,
                                 const char *own_fault, amc_fields_grid_dev *G)
{
    if (kind != AMC_FIELDS_CARTESIAN && kind != AMC_FIELDS_AXISYMMETRIC)
        return amc_fail(c, AMC_ERR_INVALID, "%s.kind %d is neither Cartesian (0) nor axisymmetric (1)", who, kind);
    if (n1 < 1 || n2 < 1 || n3 < 1 || (long long)n1 * n2 * n3 > max_bins)
        return amc_fail(c, AMC_ERR_INVALID, "%s: %d x %d x %d %s (each >= 1, at most %d in all)", who, n1, n2, n3, unit, max_bins);
    if (own_fault) return amc_fail(c, AMC_ERR_INVALID, "%s: %s", who, own_fault);
    if (kind == AMC_FIELDS_AXISYMMETRIC && (n3 != 1 || lo[0] != 0.0))
        return amc_fail(c, AMC_ERR_INVALID, "%s: an axisymmetric grid has n3 == 1 and r from lo[0] == 0", who);
    if (every < 0 || step_offset < 0 || !reserved0)
        return amc_fail(c, AMC_ERR_INVALID, "%s: every and step_offset must be >= 0, reserved 0", who);
    const int axes = kind == AMC_FIELDS_CARTESIAN ? 3 : 2;
    for (int k = 0; k < axes; k++)
        if (!(isfinite(lo[k]) && isfinite(hi[k]) && lo[k] < hi[k]))
            return amc_fail(c, AMC_ERR_INVALID, "%s: axis %d needs finite bounds lo < hi", who, k + 1);
    G->kind = kind; G->n1 = n1; G->n2 = n2; G->n3 = n3; G->bins = n1 * n2 * n3;
    const int n[3] = {n1, n2, n3};
    for (int k = 0; k < 3; k++) {       // (the unused third axis of an axisymmetric grid: [0, 1], one bin)
        G->lo[k] = k < axes ? lo[k] : 0.0;
        G->hi[k] = k < axes ? hi[k] : 1.0;
        G->w[k] = k < axes ? (hi[k] - lo[k]) / (double)n[k] : 1.0;
    }
    return AMC_OK;
}

// slab rows a sampler allocates: its environment knob `env` if set (blocks_env, else 0), else one workgroup per CU
static inline void amc_sample_blocks_config(amc_ctx *c, const char *env, int *blocks_env, int *max_blocks)
{
    *blocks_env = getenv(env) ? atoi(getenv(env)) : 0;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess || cus < 1) cus = 256;
    *max_blocks = *blocks_env > 0 ? *blocks_env : cus;
}
// workgroups of one sample of the context's index range: the knob, else one per 8,192 particles, at most max_blocks
#define AMC_SAMPLE_PER_BLOCK 8192
#define AMC_SAMPLE_MAX_PARTICLES (1LL << 24)
static inline int amc_sample_blocks(amc_ctx *c, const char *who, int blocks_env, int max_blocks, int *blocks)
{
    const long long cnt = c->hi - c->lo;
    if (cnt > AMC_SAMPLE_MAX_PARTICLES)
        return amc_fail(c, AMC_ERR_CAPACITY, "%s: %lld particles in one sample (at most 2^24 keep the sums exact)", who, cnt);
    const long long by_count = std::max<long long>(1, (cnt + AMC_SAMPLE_PER_BLOCK - 1) / AMC_SAMPLE_PER_BLOCK);
    *blocks = (int)std::min<long long>(max_blocks, blocks_env > 0 ? blocks_env : by_count);
    return AMC_OK;
}

// the kernels' view of the last sweep's deferred results, if a step left any pending
static inline amc_lazy amc_sample_lazy(const amc_ctx *c)
{
    amc_lazy L = {};
    if (c->step.lazy_pending) { L.slot_of = c->W.slot_of; L.state = c->W.sl_state; L.moved = c->W.sl_moved; L.enabled = 1; }
    return L;
}

// A sampler's running totals on the device: `words` 64-bit words of (low, high) pairs and nmeta counters, of which
// meta[bad_slot] is the error word — the lowest particle out of the quantisers' range, ~0: none.
#define AMC_TOTALS_MAX_META 8
struct amc_totals { unsigned long long *tot; size_t words; unsigned long long *meta; int nmeta, bad_slot; };
// totals (zero when nullptr) and counters in, the error word cleared; synchronises
static inline int amc_totals_put(amc_ctx *c, const amc_totals &T, const int64_t *totals, const unsigned long long *meta_init)
{
    unsigned long long meta[AMC_TOTALS_MAX_META];
    if (T.nmeta > AMC_TOTALS_MAX_META) return amc_fail(c, AMC_ERR_INVALID, "amc_totals_put: %d counters (at most %d)", T.nmeta, AMC_TOTALS_MAX_META);
    memcpy(meta, meta_init, sizeof(unsigned long long) * (size_t)T.nmeta);
    meta[T.bad_slot] = ~0ULL;
    if (totals) AMC_HIP(c, hipMemcpyAsync(T.tot, totals, sizeof(unsigned long long) * T.words, hipMemcpyHostToDevice, c->stream));
    else AMC_HIP(c, hipMemsetAsync(T.tot, 0, sizeof(unsigned long long) * T.words, c->stream));
    AMC_HIP(c, hipMemcpyAsync(T.meta, meta, sizeof(unsigned long long) * (size_t)T.nmeta, hipMemcpyHostToDevice, c->stream));
    AMC_HIP(c, hipStreamSynchronize(c->stream));
    return AMC_OK;
}
// totals (unless nullptr) and counters out through the staging buffer; synchronises.  *bad: the error word (~0: none)
static inline int amc_totals_get(amc_ctx *c, const amc_totals &T, int64_t *totals, unsigned long long *meta_out, unsigned long long *bad)
{
    amc_stage st(c);
    if (totals) AMC_HIP(c, st.get(totals, T.tot, sizeof(unsigned long long) * T.words));
    AMC_HIP(c, st.get(meta_out, T.meta, sizeof(unsigned long long) * (size_t)T.nmeta));
    AMC_HIP(c, st.finish());
    *bad = meta_out[T.bad_slot];
    return AMC_OK;
}

// The entry points of a sampler whose counters are [unused, samples, particles outside, the error word] and whose range is the
// velocity quantisers' (the fields, the fluxes, the distributions) over its totals T; c is not null: they have looked.
static inline int amc_sampler_reset(amc_ctx *c, bool on, const char *name, const amc_totals &T)
{
    if (int rc = amc_sampler_ready(c, on, name, "reset")) return rc;
    const unsigned long long meta[4] = {0, 0, 0, 0};
    return amc_totals_put(c, T, nullptr, meta);
}
static inline int amc_sampler_sample(amc_ctx *c, bool on, const char *name, int (*enqueue)(amc_ctx *c))
{
    if (int rc = amc_sampler_sample_ready(c, on, name)) return rc;
    return enqueue(c);
}
static inline int amc_sampler_read(amc_ctx *c, bool on, const char *name, const amc_totals &T, int64_t *totals, int64_t *n_samples, int64_t *n_outside)
{
    if (int rc = amc_sampler_ready(c, on, name, "read")) return rc;
    unsigned long long meta[4], bad;
    if (int rc = amc_totals_get(c, T, totals, meta, &bad)) return rc;
    if (bad != ~0ULL)
        return amc_fail(c, AMC_ERR_CAPACITY, "%s: particle %llu has a velocity component outside |c| < 2^14 m/s (or NaN); "
                        "sampling stopped until %s_reset", name, bad, name);
    if (n_samples) *n_samples = (int64_t)meta[1];
    if (n_outside) *n_outside = (int64_t)meta[2];
    return AMC_OK;
}
static inline int amc_sampler_load(amc_ctx *c, bool on, const char *name, const amc_totals &T, const int64_t *totals, int64_t n_samples, int64_t n_outside)
{
    if (!totals || n_samples < 0 || n_outside < 0) return AMC_ERR_INVALID;
    if (int rc = amc_sampler_ready(c, on, name, "load")) return rc;
    const unsigned long long meta[4] = {0, (unsigned long long)n_samples, (unsigned long long)n_outside, 0};
    return amc_totals_put(c, T, totals, meta);
}
