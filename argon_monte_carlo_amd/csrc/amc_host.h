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
AMC_INTERNAL int amc_fields_step(amc_ctx *c);                         // the fields' part of the cadence hook (amc_fields.hip)
AMC_INTERNAL int amc_corr_step(amc_ctx *c);                           // the correlations' part (amc_corr.hip)

// amc_timestep, amc_run and the stage calls: not in the middle of a sharded step (the rule above amc_mg_step)
static inline int amc_mg_step_idle(amc_ctx *c, const char *who)
{
    if (c->MG.step.phase == AMC_MG_IDLE) return AMC_OK;
    return amc_fail(c, AMC_ERR_STATE, "%s in the middle of a sharded step (amc_mg_pack ... amc_mg_finish): finish it, or start over with "
                                      "amc_mg_local / amc_upload", who);
}

// a sample is due after the step that leaves the step counter at `step`
static inline bool amc_fields_due(const amc_ctx *c, int64_t step)
{
    return c->F.on && c->F.g.every > 0 && (step + c->F.g.step_offset) % c->F.g.every == 0;
}
static inline bool amc_corr_due(const amc_ctx *c, int64_t step)
{
    return c->CR.on && c->CR.g.every > 0 && (step + c->CR.g.step_offset) % c->CR.g.every == 0;
}
// ... for any sampler of the particle state: such a step ends with the state everybody reads (no deferred bounds pass)
static inline bool amc_samplers_due(const amc_ctx *c, int64_t step) { return amc_fields_due(c, step) || amc_corr_due(c, step); }
// a sampler runs on a cadence: amc_run takes its plain loop
static inline bool amc_samplers_cadence(const amc_ctx *c) { return (c->F.on && c->F.g.every > 0) || (c->CR.on && c->CR.g.every > 0); }
// the cadence hook after a completed step
static inline int amc_samplers_step(amc_ctx *c)
{
    if (int rc = amc_fields_step(c)) return rc;
    return c->CR.on ? amc_corr_step(c) : AMC_OK;
}
