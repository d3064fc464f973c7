// amc_transit.hip — sampled transits: entries into, exits from and residence times in up to eight zones, with a memory per
// particle (include/argonmc_transit.h).  The reference has no such output; the Python layer derives transmission
// probabilities, residence times, rates and occupancies from the totals.
//
// One sample is two kernels, the streaming samplers' pair (amc_sample_dev.h):
//   k_transit_accum   a persistent grid of at most one workgroup per CU.  Each workgroup streams a contiguous index range: the
//                     coordinate arrays of the axes in use (8 B each, 16-B loads of particle pairs) and the particles' state
//                     words (4 B, 8-B loads).  A particle's new position word is built from compares alone; where it equals
//                     the stored one — the common case — nothing else happens but a per-lane count of the zones it is inside.
//                     Where it differs (a few particles per thousand) the particle goes into a queue in LDS, and the stream
//                     goes on: the queue is worked off after the walk, one event per lane, all of a workgroup's dependent,
//                     scattered accesses in flight together — the changed zones are walked: entry-index array, LDS atomics
//                     whose result nobody reads into a table of 64-bit columns, the state word stored back.  (A full queue —
//                     the first sample after a reset, when everybody is seen for the first time — handles the event in
//                     place.)  The table leaves as one slab row with plain stores — no global atomics but the atomicMin on
//                     the error word.
//   k_slab_reduce<unsigned long long, transit_sink>  sums the slab rows per column; the sink adds the result into the 128-bit
//                     running totals, the two limbs of sum_tau2 into one total (the reduce's companion column), and nothing
//                     once the error word or the sample limit's flag is set.
// Integer sums do not depend on the order of the adds, so the totals are bitwise the same for any number of workgroups.
#include "amc_host.h"
#include "amc_sample_dev.h"

#define AMC_TRANSIT_THREADS 512
#define TR_QUEUE 4096                   // events a workgroup defers to the end of its walk: 32 KiB of LDS
// a slab row's columns per zone: the totals' (argonmc_transit.h) with sum_tau2 as two columns, the sums of tau * tau's low and
// high 32-bit limbs
#define TR_CLASS (AMC_TRANSIT_CLASS_COLUMNS + 1)
#define TR_COLUMNS (5 + 6 * TR_CLASS)
// Why 64-bit columns are exact within a launch: amc_sample_blocks refuses a sample of more than AMC_SAMPLE_MAX_PARTICLES = 2^24
// particles, a particle adds to a column of a zone at most once per sample, and what it adds is 1, tau or a 32-bit limb of
// tau * tau — each below 2^32, since the sample index is at most AMC_TRANSIT_MAX_SAMPLES - 1 = 2^32 - 2.  So a column of a table,
// and its sum over the slab rows, stays below 2^24 * 2^32 = 2^56: far from wrapping, and non-negative as amc_add128 reads it.
static_assert(AMC_SAMPLE_MAX_PARTICLES <= (1LL << 24) && AMC_TRANSIT_MAX_SAMPLES <= (1LL << 32) - 1, "a launch's column sums stay below 2^56");
static_assert(AMC_TRANSIT_COLUMNS == 5 + 6 * AMC_TRANSIT_CLASS_COLUMNS && AMC_TRANSIT_CLASS_COLUMNS == 3 + AMC_TRANSIT_HIST, "the totals' layout");
static_assert(AMC_TRANSIT_MAX_ZONES * 4 == 32, "four bits per zone in one 32-bit state word");

// the zones as the kernel takes them
struct amc_transit_dev {
    int n_zones, used;                  // used: bit a set if some zone looks at axis a
    int axis[AMC_TRANSIT_MAX_ZONES];
    double lo[AMC_TRANSIT_MAX_ZONES], hi[AMC_TRANSIT_MAX_ZONES];
};

AMC_DEV void tr_add(unsigned long long *p, unsigned long long v) { (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// The position word of one particle: per zone 1 below, 2 inside, 3 above (zones beyond n_zones: 0).  *nan: a coordinate in use
// is NaN.
AMC_DEV unsigned int tr_positions(const amc_transit_dev &T, double x, double y, double z, bool *nan)
{
    unsigned int w = 0;
    bool bad = false;
#pragma unroll
    for (int k = 0; k < AMC_TRANSIT_MAX_ZONES; k++) {
        if (k >= T.n_zones) break;
        const double u = T.axis[k] == 0 ? x : T.axis[k] == 1 ? y : z;
        bad = bad || u != u;
        w |= (u < T.lo[k] ? 1u : u < T.hi[k] ? 2u : 3u) << (4 * k);
    }
    *nan = bad;
    return w;
}

// The rare path: the zones of particle p whose position changed (ow: the stored state word, nw: the new position word).
// Returns the new state word.
AMC_DEV unsigned int tr_events(unsigned long long *tab, unsigned int *entry, long long stride, long long p, unsigned int s, unsigned int ow,
                               unsigned int nw)
{
    unsigned int w = ow;
    unsigned int m = (ow ^ nw) & 0x33333333u;
    while (m) {
        const int k = (__ffs((int)m) - 1) >> 2;
        const unsigned int a = (ow >> (4 * k)) & 3u, b = (nw >> (4 * k)) & 3u;
        m &= ~(0xFu << (4 * k));
        w &= ~(0xFu << (4 * k));
        unsigned long long *t = tab + k * TR_COLUMNS;
        auto *e = amc_g(entry) + (size_t)k * (size_t)stride + p;
        if (b == 2u) {                  // an entry: from below, from above, or inside when first seen
            const unsigned int side = a == 0u ? 2u : (a - 1u) >> 1;
            tr_add(t + side, 1ULL);
            *e = s;
            w |= (2u | side << 2) << (4 * k);
        } else if (a == 2u) {           // an exit of class (entry side, exit side)
            const unsigned int side = min((ow >> (4 * k + 2)) & 3u, 2u);
            const unsigned int tau = s - *e;
            const unsigned long long tau2 = (unsigned long long)tau * tau;
            unsigned long long *c = t + 5 + (2 * side + (b >> 1)) * TR_CLASS;
            tr_add(c, 1ULL);
            tr_add(c + 1, tau);
            tr_add(c + 2, tau2 & 0xFFFFFFFFULL);
            tr_add(c + 3, tau2 >> 32);
            const int col = tau ? 31 - __clz((int)tau) : 0;     // (tau >= 1 — the sample limit keeps it below 2^32: columns 0 .. 31)
            tr_add(c + 4 + (col < AMC_TRANSIT_HIST ? col : AMC_TRANSIT_HIST - 1), 1ULL);
            w |= b << (4 * k);
        } else {                        // first seen outside, or a crossing no sample saw
            if (a != 0u) tr_add(t + 3, 1ULL);
            w |= b << (4 * k);
        }
    }
    return w;
}

// meta: [0] unused, [1] samples, [2] != 0: a sample beyond the limit was asked for, [3] lowest particle with a NaN coordinate (~0: none)
__global__ __launch_bounds__(AMC_TRANSIT_THREADS) void k_transit_accum(amc_state S, amc_lazy L, long long lo, long long hi, amc_transit_dev T,
                                                                       unsigned int *state, unsigned int *entry, long long stride,
                                                                       unsigned long long *slab, unsigned long long *meta)
{
    __shared__ unsigned long long tab[AMC_TRANSIT_MAX_ZONES * TR_COLUMNS];
    __shared__ unsigned long long head[2];
    __shared__ uint2 queue[TR_QUEUE];   // (particle index - lo, new position word) of the particles with an event
    __shared__ unsigned int queued;
    const int M = T.n_zones * TR_COLUMNS;
    // (one read per workgroup: another workgroup of this sample may set the error word meanwhile, and all threads must agree)
    if (threadIdx.x == 0) { head[0] = amc_g(meta)[1]; head[1] = amc_g(meta)[3]; queued = 0; }
    amc_slab_begin(tab, M);
    // a stopped sampler changes nothing, the particles' state included
    const unsigned long long ns = head[0];
    if (head[1] != ~0ULL) return;
    if (ns >= (unsigned long long)AMC_TRANSIT_MAX_SAMPLES) {
        if (blockIdx.x == 0 && threadIdx.x == 0) amc_g(meta)[2] = 1ULL;
        return;
    }
    const unsigned int s = (unsigned int)ns;
    const auto *gx = amc_g(S.x), *gy = amc_g(S.y), *gz = amc_g(S.z);
    auto *gs = amc_g(state);
    unsigned int inside[AMC_TRANSIT_MAX_ZONES];
#pragma unroll
    for (int k = 0; k < AMC_TRANSIT_MAX_ZONES; k++) inside[k] = 0;
    long long first_bad = -1;
    // per pair one 16-byte load per coordinate array in use and one 8-byte load of the state words
    for (amc_sample_walk w(lo, hi); w.more(); w.next()) {
        const long long p0 = w.p0();
        const bool v0 = w.v0(), v1 = w.v1();
        double x[2] = {0.0, 0.0}, y[2] = {0.0, 0.0}, z[2] = {0.0, 0.0};
        unsigned int ow[2];
        if (v0 && v1) {
            if (T.used & 1) { const double2 a = amc_g_load((const double2 *)(S.x + p0)); x[0] = a.x; x[1] = a.y; }
            if (T.used & 2) { const double2 a = amc_g_load((const double2 *)(S.y + p0)); y[0] = a.x; y[1] = a.y; }
            if (T.used & 4) { const double2 a = amc_g_load((const double2 *)(S.z + p0)); z[0] = a.x; z[1] = a.y; }
            const uint2 o = amc_g_load((const uint2 *)(state + p0));
            ow[0] = o.x; ow[1] = o.y;
        } else {
            const long long p = v0 ? p0 : p0 + 1;
            const int e = v0 ? 0 : 1;
            if (T.used & 1) x[e] = gx[p];
            if (T.used & 2) y[e] = gy[p];
            if (T.used & 4) z[e] = gz[p];
            ow[e] = gs[p];
            ow[1 - e] = 0;
        }
#pragma unroll
        for (int e = 0; e < 2; e++) {
            if (!(e == 0 ? v0 : v1)) continue;
            const long long p = p0 + e;
            double vx, vy, vz;          // (not looked at: their loads fall away)
            amc_fields_lazy(L, p, x[e], y[e], z[e], vx, vy, vz);
            bool nan;
            const unsigned int nw = tr_positions(T, x[e], y[e], z[e], &nan);
            if (nan) {
                if (first_bad < 0) first_bad = p;
                continue;
            }
            const unsigned int in = (nw >> 1) & ~nw & 0x11111111u;      // one bit per zone the particle is inside
#pragma unroll
            for (int q = 0; q < AMC_TRANSIT_MAX_ZONES; q++) inside[q] += (in >> (4 * q)) & 1u;
            if ((ow[e] ^ nw) & 0x33333333u) {
                const unsigned int slot = atomicAdd(&queued, 1u);
                if (slot < TR_QUEUE) queue[slot] = make_uint2((unsigned int)(p - lo), nw);
                else gs[p] = tr_events(tab, entry, stride, p, s, ow[e], nw);
            }
        }
    }
    // the deferred events: every particle is queued at most once per sample and belongs to this workgroup alone, so its stored
    // word is still the one the walk read
    __syncthreads();
    const unsigned int nq = queued < TR_QUEUE ? queued : TR_QUEUE;
    for (unsigned int i = threadIdx.x; i < nq; i += blockDim.x) {
        const uint2 q = queue[i];
        const long long p = lo + (long long)q.x;
        gs[p] = tr_events(tab, entry, stride, p, s, gs[p], q.y);
    }
#pragma unroll
    for (int q = 0; q < AMC_TRANSIT_MAX_ZONES; q++)
        if (q < T.n_zones && inside[q]) tr_add(tab + q * TR_COLUMNS + 4, inside[q]);
    if (first_bad >= 0) (void)__hip_atomic_fetch_min(amc_g(meta) + 3, (unsigned long long)first_bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    amc_slab_store(slab, tab, M);
}

// (lo, hi) += v * 2^32 for a non-negative v below 2^64: the high limb of sum_tau2
AMC_DEV void tr_add128_limb1(unsigned long long &lo, unsigned long long &hi, unsigned long long v)
{
    const unsigned long long now = lo + (v << 32);
    hi += (v >> 32) + (now < lo ? 1ULL : 0ULL);
    lo = now;
}

// The transits' end of k_slab_reduce: column j of the slab is (zone, slab column) and goes with carry into the 128-bit totals.  The
// thread of a sum_tau2 low-limb column has the high limb's sum, the column beside it, as its companion and adds both into the one
// total; the high limb's own thread does nothing (two threads must not add into the same total).  Sums stay below 2^56: above.
struct transit_sink {
    static constexpr bool companion = true;
    unsigned long long *tot, *meta;
    // the column of its exit class that slab column j is (2: sum_tau2's low limb, 3: its high limb), -1: one of the zone's first five
    AMC_DEV static int class_column(int j) { const int c = j % TR_COLUMNS; return c < 5 ? -1 : (c - 5) % TR_CLASS; }
    AMC_DEV bool stopped() const { return amc_g(meta)[3] != ~0ULL || amc_g(meta)[2] != 0ULL; }     // (the read reports it)
    AMC_DEV int stride(int W) const { return W; }
    AMC_DEV int mate(int j) const { const int q = class_column(j); return q == 2 ? 1 : q == 3 ? -1 : 0; }
    template <class Mate>
    AMC_DEV void column(int j, unsigned long long s, Mate mate_sum) const
    {
        const int zone = j / TR_COLUMNS, c = j % TR_COLUMNS, q = class_column(j);
        const int k = c < 5 ? 0 : (c - 5) / TR_CLASS;       // the exit class
        auto *t = amc_g(tot) + 2 * ((size_t)zone * AMC_TRANSIT_COLUMNS + (c < 5 ? c : 5 + k * AMC_TRANSIT_CLASS_COLUMNS + (q < 3 ? q : q - 1)));
        unsigned long long tl = t[0], th = t[1];
        amc_add128(tl, th, s);
        if (q == 2) tr_add128_limb1(tl, th, mate_sum());
        t[0] = tl; t[1] = th;
    }
    AMC_DEV void counters(unsigned long long) const { amc_g(meta)[1] += 1; }
};

// ---- the host side -------------------------------------------------------------------------------------------------------------
int amc_transit_enqueue(amc_ctx *c)    // (AMC_INTERNAL: the cadence hook's)
{
    amc_transit_ws &F = c->TR;
    int blocks;
    if (int rc = amc_sample_blocks(c, "amc_transit", F.blocks_env, F.max_blocks, &blocks)) return rc;
    amc_transit_dev T = {};
    T.n_zones = F.g.n_zones;
    for (int k = 0; k < F.g.n_zones; k++) {
        T.axis[k] = F.g.axis[k]; T.lo[k] = F.g.lo[k]; T.hi[k] = F.g.hi[k];
        T.used |= 1 << F.g.axis[k];
    }
    const int W = F.g.n_zones * TR_COLUMNS;
    amc_prof_begin(c, AMC_K_FIELDS);
    AMC_LAUNCH(c, k_transit_accum, dim3(blocks), dim3(AMC_TRANSIT_THREADS), c->S, amc_sample_lazy(c), (long long)c->lo, (long long)c->hi, T, F.state,
               F.entry, (long long)F.stride, F.slab, F.meta);
    amc_prof_end(c);
    AMC_HIP(c, hipGetLastError());
    AMC_HIP(c, amc_launch_slab_reduce(c, (const unsigned long long *)F.slab, blocks, W, transit_sink{F.tot, F.meta}));
    return AMC_OK;
}

static void transit_free(amc_ctx *c)
{
    ctx_free(c, c->TR.slab, c->TR.tot, c->TR.meta, c->TR.state, c->TR.entry);
    c->TR = amc_transit_ws();
}

static amc_totals transit_totals(const amc_transit_ws &F) { return amc_totals{F.tot, (size_t)2 * AMC_TRANSIT_COLUMNS * (size_t)F.g.n_zones, F.meta, 4, 3}; }

// a state word as the kernel leaves it: per zone in use a position 0 .. 3 and, only while inside, an entry side 0 .. 2
static bool transit_word_ok(uint32_t w, int n_zones)
{
    for (int k = 0; k < AMC_TRANSIT_MAX_ZONES; k++) {
        const uint32_t pos = (w >> (4 * k)) & 3u, side = (w >> (4 * k + 2)) & 3u;
        if (k >= n_zones ? (pos | side) != 0 : side > 2u || (pos != 2u && side != 0u)) return false;
    }
    return true;
}

extern "C" {

int amc_transit_reset(amc_ctx *c)
{
    if (!c) return AMC_ERR_INVALID;
    if (int rc = amc_sampler_ready(c, c->TR.on, "amc_transit", "reset")) return rc;
    amc_transit_ws &F = c->TR;
    AMC_HIP(c, hipMemsetAsync(F.state, 0, sizeof(unsigned int) * (size_t)F.stride, c->stream));
    AMC_HIP(c, hipMemsetAsync(F.entry, 0, sizeof(unsigned int) * (size_t)F.stride * (size_t)F.g.n_zones, c->stream));
    const unsigned long long meta[4] = {0, 0, 0, 0};
    return amc_totals_put(c, transit_totals(F), nullptr, meta);
}

int amc_transit_config(amc_ctx *c, const amc_transit_grid *g)
{
    bool done;
    if (int rc = amc_sampler_config_begin(c, g, "amc_transit_grid", transit_free, &done); rc || done) return rc;
    if (g->n_zones < 1 || g->n_zones > AMC_TRANSIT_MAX_ZONES)
        return amc_fail(c, AMC_ERR_INVALID, "amc_transit_grid: %d zones (1 .. %d)", g->n_zones, AMC_TRANSIT_MAX_ZONES);
    if (g->every < 0 || g->step_offset < 0 || g->reserved[0] != 0 || g->reserved[1] != 0)
        return amc_fail(c, AMC_ERR_INVALID, "amc_transit_grid: every and step_offset must be >= 0, reserved 0");
    for (int k = 0; k < AMC_TRANSIT_MAX_ZONES; k++) {
        if (k >= g->n_zones) {
            if (g->axis[k] != 0 || g->lo[k] != 0.0 || g->hi[k] != 0.0)
                return amc_fail(c, AMC_ERR_INVALID, "amc_transit_grid: zone %d is beyond n_zones: axis, lo and hi must be 0", k);
            continue;
        }
        if (g->axis[k] < 0 || g->axis[k] > 2) return amc_fail(c, AMC_ERR_INVALID, "amc_transit_grid: zone %d has axis %d (0, 1 or 2)", k, g->axis[k]);
        if (!(isfinite(g->lo[k]) && isfinite(g->hi[k]) && g->lo[k] < g->hi[k]))
            return amc_fail(c, AMC_ERR_INVALID, "amc_transit_grid: zone %d needs finite bounds lo < hi", k);
    }
    transit_free(c);
    amc_transit_ws &F = c->TR;
    F.g = *g;
    amc_sample_blocks_config(c, "AMC_TRANSIT_BLOCKS", &F.blocks_env, &F.max_blocks);
    F.stride = (std::max<int64_t>(c->n, 1) + 1) & ~(int64_t)1;
    if (dalloc(c, &F.slab, (size_t)F.max_blocks * (size_t)g->n_zones * TR_COLUMNS) != hipSuccess || dalloc(c, &F.tot, transit_totals(F).words) != hipSuccess ||
        dalloc(c, &F.meta, 4) != hipSuccess || dalloc(c, &F.state, (size_t)F.stride) != hipSuccess ||
        dalloc(c, &F.entry, (size_t)F.stride * (size_t)g->n_zones) != hipSuccess) {
        transit_free(c);
        return amc_fail(c, AMC_ERR_HIP, "amc_transit_config: device allocation failed");
    }
    F.on = true;
    if (int rc = amc_transit_reset(c)) { transit_free(c); return rc; }
    return AMC_OK;
}

int amc_transit_sample(amc_ctx *c)
{
    if (!c) return AMC_ERR_INVALID;
    if (int rc = amc_sampler_sample_ready(c, c->TR.on, "amc_transit")) return rc;
    return amc_transit_enqueue(c);
}

int amc_transit_read(amc_ctx *c, int64_t *totals, int64_t *n_samples)
{
    if (!c) return AMC_ERR_INVALID;
    if (int rc = amc_sampler_ready(c, c->TR.on, "amc_transit", "read")) return rc;
    unsigned long long meta[4], bad;
    if (int rc = amc_totals_get(c, transit_totals(c->TR), totals, meta, &bad)) return rc;
    if (bad != ~0ULL)
        return amc_fail(c, AMC_ERR_CAPACITY, "amc_transit: particle %llu has a NaN coordinate; sampling stopped until amc_transit_reset", bad);
    if (meta[2] != 0)
        return amc_fail(c, AMC_ERR_CAPACITY, "amc_transit: a sample beyond the limit of 2^32 - 1 samples was asked for; sampling stopped until "
                                             "amc_transit_reset");
    if (n_samples) *n_samples = (int64_t)meta[1];
    return AMC_OK;
}

int amc_transit_state(amc_ctx *c, uint32_t *state, uint32_t *entry)
{
    if (!c) return AMC_ERR_INVALID;
    if (int rc = amc_sampler_ready(c, c->TR.on, "amc_transit", "state")) return rc;
    amc_transit_ws &F = c->TR;
    const size_t cnt = (size_t)(c->hi - c->lo), bytes = sizeof(uint32_t) * cnt;
    if (state && bytes) AMC_HIP(c, hipMemcpyAsync(state, F.state + c->lo, bytes, hipMemcpyDeviceToHost, c->stream));
    for (int k = 0; k < F.g.n_zones; k++)
        if (entry && bytes) AMC_HIP(c, hipMemcpyAsync(entry + (size_t)k * cnt, F.entry + (size_t)k * (size_t)F.stride + c->lo, bytes, hipMemcpyDeviceToHost, c->stream));
    AMC_HIP(c, hipStreamSynchronize(c->stream));
    return AMC_OK;
}

int amc_transit_load(amc_ctx *c, const int64_t *totals, int64_t n_samples, const uint32_t *state, const uint32_t *entry)
{
    if (!c || !totals) return AMC_ERR_INVALID;
    if (int rc = amc_sampler_ready(c, c->TR.on, "amc_transit", "load")) return rc;
    amc_transit_ws &F = c->TR;
    if (n_samples < 0 || n_samples > AMC_TRANSIT_MAX_SAMPLES)
        return amc_fail(c, AMC_ERR_INVALID, "amc_transit_load: %lld samples (0 .. 2^32 - 1)", (long long)n_samples);
    const size_t cnt = (size_t)(c->hi - c->lo), bytes = sizeof(uint32_t) * cnt;
    for (size_t p = 0; state && p < cnt; p++)
        if (!transit_word_ok(state[p], F.g.n_zones))
            return amc_fail(c, AMC_ERR_INVALID, "amc_transit_load: state word 0x%08x of particle %lld is none a sample leaves", state[p],
                            (long long)(c->lo + (int64_t)p));
    const unsigned long long meta[4] = {0, (unsigned long long)n_samples, 0, 0};
    if (int rc = amc_totals_put(c, transit_totals(F), totals, meta)) return rc;
    if (state) { if (bytes) AMC_HIP(c, hipMemcpyAsync(F.state + c->lo, state, bytes, hipMemcpyHostToDevice, c->stream)); }
    else AMC_HIP(c, hipMemsetAsync(F.state, 0, sizeof(unsigned int) * (size_t)F.stride, c->stream));
    for (int k = 0; k < F.g.n_zones; k++) {
        unsigned int *dst = F.entry + (size_t)k * (size_t)F.stride;
        if (entry) { if (bytes) AMC_HIP(c, hipMemcpyAsync(dst + c->lo, entry + (size_t)k * cnt, bytes, hipMemcpyHostToDevice, c->stream)); }
        else AMC_HIP(c, hipMemsetAsync(dst, 0, sizeof(unsigned int) * (size_t)F.stride, c->stream));
    }
    AMC_HIP(c, hipStreamSynchronize(c->stream));
    return AMC_OK;
}

}  // extern "C"
