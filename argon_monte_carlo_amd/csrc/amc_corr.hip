// amc_corr.hip — sampled correlations: per group and lag, the particle count, the squared displacement components and the
// velocity products against a stored time origin, accumulated as exact integers (include/argonmc.h "sampled correlations",
// DESIGN.md 12).  The reference has no such output; the Python layer derives the mean-square displacement, the velocity
// autocorrelation function and diffusion coefficients from the totals.
//
// One sample is two kernels, the streaming samplers' pair (amc_sample_dev.h):
//   k_corr_accum<MODE>  a persistent grid of at most one workgroup per CU, each over a contiguous index range, 16-byte loads
//                       of particle pairs.  MODE origin: 48 B of state per particle in, 48 B of origin out, lag 0.  MODE lag:
//                       state and origin in (96 B), the launch's lag.  MODE lag-and-origin: the last lag of the window against
//                       the old origin, the new origin out, lag 0 — one pass.  The lag is uniform per launch, so the table in
//                       LDS is groups x 7 int64 (two of them in the last mode: 28 KiB at most).  A lane keeps a running
//                       (group, 7 sums) in registers and flushes it to LDS (64-bit integer LDS atomics) only when the group
//                       changes and at the end: with one group every lane would otherwise hit the same seven words.  The
//                       table leaves as one slab row with plain stores — no global atomics but the atomicMin on the error word.
//   k_slab_reduce<unsigned long long, sample_sink>  (amc_fields.hip: the fields' sink) sums the slab rows per (group, quantity)
//                       into the 128-bit totals at the launch's lag or lags, with carry, and bumps the counters.
// The walk, the pair loads and stores, the group rule (amc_sample_bin), the speed test and the lazy read are amc_sample_dev.h's.
#include "amc_host.h"
#include "amc_sample_dev.h"

#define AMC_CORR_Q AMC_SAMPLE_Q          // count, m(x y z), c(x y z)
#define AMC_CORR_THREADS 512            // 8 waves per CU: the lag-and-origin instance needs more than the 128 VGPRs 16 waves leave
#define AMC_CORR_ORIGIN 0
#define AMC_CORR_LAG 1
#define AMC_CORR_LAG_ORIGIN 2

struct amc_corr_arrays {
    double *x, *y, *z, *vx, *vy, *vz;
};

// a lane's running sums of one group
struct corr_run {
    int g;
    unsigned long long s[AMC_CORR_Q];
};

AMC_DEV void corr_flush(unsigned long long *tab, const corr_run &r)
{
    if (r.g < 0) return;
    unsigned long long *t = tab + (size_t)r.g * AMC_CORR_Q;
#pragma unroll
    for (int q = 0; q < AMC_CORR_Q; q++)
        if (r.s[q]) atomicAdd(t + q, r.s[q]);
}

AMC_DEV void corr_enter(unsigned long long *tab, corr_run &r, int g)
{
    if (g == r.g) return;
    corr_flush(tab, r);
    r.g = g;
#pragma unroll
    for (int q = 0; q < AMC_CORR_Q; q++) r.s[q] = 0;
}

AMC_DEV unsigned long long corr_m(double d) { return (unsigned long long)(long long)rint(ldexp(d * d, 74)); }
AMC_DEV unsigned long long corr_c(double v, double v0) { return (unsigned long long)(long long)rint((v * v0) * 1024.0); }

// one particle at lag 0 (its own origin); false: a component out of the quantisation range
AMC_DEV bool corr_origin_particle(const amc_fields_grid_dev &G, unsigned long long *tab, corr_run &r, unsigned int &outside, double x,
                                  double y, double z, double vx, double vy, double vz)
{
    const int g = amc_sample_bin(G, x, y, z);
    if (g < 0) { outside++; return true; }
    if (!amc_sample_speed_ok(vx, vy, vz)) return false;
    corr_enter(tab, r, g);
    r.s[0] += 1ULL;
    r.s[4] += corr_c(vx, vx);
    r.s[5] += corr_c(vy, vy);
    r.s[6] += corr_c(vz, vz);
    return true;
}

// one particle against its stored origin
AMC_DEV bool corr_lag_particle(const amc_fields_grid_dev &G, unsigned long long *tab, corr_run &r, double x, double y, double z,
                               double vx, double vy, double vz, double x0, double y0, double z0, double vx0, double vy0, double vz0)
{
    const int g = amc_sample_bin(G, x0, y0, z0);
    if (g < 0) return true;             // (no part in this window: counted when the origin was stored)
    const double ex = x - x0, ey = y - y0, ez = z - z0;
    const double lim = 3.814697265625e-06;      // 2^-18
    if (!(fabs(ex) < lim && fabs(ey) < lim && fabs(ez) < lim) || !amc_sample_speed_ok(vx, vy, vz) || !amc_sample_speed_ok(vx0, vy0, vz0)) return false;
    corr_enter(tab, r, g);
    r.s[0] += 1ULL;
    r.s[1] += corr_m(ex);
    r.s[2] += corr_m(ey);
    r.s[3] += corr_m(ez);
    r.s[4] += corr_c(vx, vx0);
    r.s[5] += corr_c(vy, vy0);
    r.s[6] += corr_c(vz, vz0);
    return true;
}

// Slab row of a workgroup: [tables][groups * 7] sums, then the particles outside.  MODE origin: one table (lag 0); MODE lag: one
// table (the launch's lag); MODE lag-and-origin: table 0 the last lag against the old origin, table 1 lag 0 of the new one.
template <int MODE>
__global__ __launch_bounds__(AMC_CORR_THREADS) void k_corr_accum(amc_state S, amc_lazy L, amc_corr_arrays O, long long lo, long long hi,
                                                                 amc_fields_grid_dev G, unsigned long long *slab, unsigned long long *bad)
{
    constexpr int TABLES = MODE == AMC_CORR_LAG_ORIGIN ? 2 : 1;
    constexpr bool LAG = MODE != AMC_CORR_ORIGIN, ORIGIN = MODE != AMC_CORR_LAG;
    __shared__ unsigned long long tab[TABLES * AMC_CORR_MAX_GROUPS * AMC_CORR_Q];
    __shared__ unsigned int outside_sum;
    const int M = G.bins * AMC_CORR_Q;
    amc_slab_begin(tab, TABLES * M, &outside_sum);
    unsigned long long *tab_lag = tab, *tab_org = tab + (TABLES - 1) * M;
    unsigned int outside = 0;
    long long first_bad = -1;
    corr_run rl, ro;
    rl.g = -1; ro.g = -1;
#pragma unroll
    for (int q = 0; q < AMC_CORR_Q; q++) { rl.s[q] = 0; ro.s[q] = 0; }
    for (amc_sample_walk w(lo, hi); w.more(); w.next()) {
        const long long p0 = w.p0();
        const bool v0 = w.v0(), v1 = w.v1();
        double x[2], y[2], z[2], vx[2], vy[2], vz[2];
        double x0[2], y0[2], z0[2], vx0[2], vy0[2], vz0[2];
        if (v0 && v1) {                 // (the state's loads and the origins' under one branch: amc_sample_dev.h)
            amc_sample_load_both(S, p0, x, y, z, vx, vy, vz);
            if (LAG) amc_sample_load_both(O, p0, x0, y0, z0, vx0, vy0, vz0);
        } else {
            amc_sample_load_one(S, v0 ? p0 : p0 + 1, v0 ? 0 : 1, x, y, z, vx, vy, vz);
            if (LAG) amc_sample_load_one(O, v0 ? p0 : p0 + 1, v0 ? 0 : 1, x0, y0, z0, vx0, vy0, vz0);
        }
#pragma unroll
        for (int e = 0; e < 2; e++) {
            if (!(e == 0 ? v0 : v1)) continue;
            const long long p = p0 + e;
            amc_fields_lazy(L, p, x[e], y[e], z[e], vx[e], vy[e], vz[e]);
            bool ok = true;
            if (LAG) ok = corr_lag_particle(G, tab_lag, rl, x[e], y[e], z[e], vx[e], vy[e], vz[e], x0[e], y0[e], z0[e], vx0[e], vy0[e], vz0[e]);
            if (ORIGIN) ok = corr_origin_particle(G, tab_org, ro, outside, x[e], y[e], z[e], vx[e], vy[e], vz[e]) && ok;
            if (!ok && first_bad < 0) first_bad = p;
        }
        if (ORIGIN) amc_sample_store_pair(O, p0, v0, v1, x, y, z, vx, vy, vz);
    }
    if (LAG) corr_flush(tab_lag, rl);
    if (ORIGIN) corr_flush(tab_org, ro);
    if (outside) atomicAdd(&outside_sum, outside);
    if (first_bad >= 0) atomicMin(bad, (unsigned long long)first_bad);
    amc_slab_store(slab, tab, TABLES * M, &outside_sum);
}

static amc_corr_arrays corr_arrays(const amc_corr_ws &R)
{
    amc_corr_arrays O;
    O.x = R.origin; O.y = R.origin + R.stride; O.z = R.origin + 2 * R.stride;
    O.vx = R.origin + 3 * R.stride; O.vy = R.origin + 4 * R.stride; O.vz = R.origin + 5 * R.stride;
    return O;
}

// one sample at the window position; advances it
static int corr_enqueue(amc_ctx *c)
{
    amc_corr_ws &R = c->CR;
    int blocks;
    if (int rc = amc_sample_blocks(c, "amc_corr", R.blocks_env, R.max_blocks, &blocks)) return rc;
    const amc_lazy L = amc_sample_lazy(c);
    const amc_fields_grid_dev &G = R.G;
    const amc_corr_arrays O = corr_arrays(R);
    const int mode = R.pos == 0 ? AMC_CORR_ORIGIN : R.pos < R.g.n_lags ? AMC_CORR_LAG : AMC_CORR_LAG_ORIGIN;
    amc_prof_begin(c, AMC_K_FIELDS);
    if (mode == AMC_CORR_ORIGIN)
        AMC_LAUNCH(c, k_corr_accum<AMC_CORR_ORIGIN>, dim3(blocks), dim3(AMC_CORR_THREADS), c->S, L, O, (long long)c->lo, (long long)c->hi, G, R.slab, R.meta + 3);
    else if (mode == AMC_CORR_LAG)
        AMC_LAUNCH(c, k_corr_accum<AMC_CORR_LAG>, dim3(blocks), dim3(AMC_CORR_THREADS), c->S, L, O, (long long)c->lo, (long long)c->hi, G, R.slab, R.meta + 3);
    else
        AMC_LAUNCH(c, k_corr_accum<AMC_CORR_LAG_ORIGIN>, dim3(blocks), dim3(AMC_CORR_THREADS), c->S, L, O, (long long)c->lo, (long long)c->hi, G, R.slab, R.meta + 3);
    amc_prof_end(c);
    AMC_HIP(c, hipGetLastError());
    // table 0 at the window position; the lag-and-origin pass has a second table, the new origin's lag 0
    AMC_HIP(c, amc_launch_sample_reduce(c, R.slab, blocks, G.bins * AMC_CORR_Q, mode == AMC_CORR_LAG_ORIGIN ? 2 : 1, (int)R.pos, 0,
                                        R.g.n_lags + 1, mode == AMC_CORR_LAG ? 0 : 1, R.tot, R.meta));
    R.pos = mode == AMC_CORR_LAG ? R.pos + 1 : 1;
    return AMC_OK;
}

// meta: [0] origins, [1] samples, [2] particles outside, [3] the error word
static amc_totals corr_totals(const amc_corr_ws &R)
{
    return amc_totals{R.tot, (size_t)2 * AMC_CORR_Q * (size_t)R.G.bins * (size_t)(R.g.n_lags + 1), R.meta, 4, 3};
}

static void corr_free(amc_ctx *c)
{
    ctx_free(c, c->CR.slab, c->CR.tot, c->CR.meta, c->CR.origin);
    c->CR = amc_corr_ws();
}

extern "C" {

int amc_corr_step(amc_ctx *c) { return corr_enqueue(c); }

int amc_corr_config(amc_ctx *c, const amc_corr_grid *g)
{
    bool done;
    if (int rc = amc_sampler_config_begin(c, g, "amc_corr_grid", corr_free, &done); rc || done) return rc;
    char lags_fault[96] = "";           // (reported behind the group count, as before the grid check was shared)
    if (g->n_lags < 1 || (long long)g->n1 * g->n2 * g->n3 * ((long long)g->n_lags + 1) > AMC_CORR_MAX_CELLS)
        snprintf(lags_fault, sizeof lags_fault, "n_lags %d (>= 1, groups * (n_lags + 1) at most %d)", g->n_lags, AMC_CORR_MAX_CELLS);
    amc_fields_grid_dev G;
    if (int rc = amc_sample_grid_check(c, "amc_corr_grid", "groups", g->kind, g->n1, g->n2, g->n3, AMC_CORR_MAX_GROUPS, g->lo, g->hi, g->every,
                                       g->step_offset, g->reserved[0] == 0 && g->reserved[1] == 0, lags_fault[0] ? lags_fault : nullptr, &G))
        return rc;
    corr_free(c);
    amc_corr_ws &R = c->CR;
    R.g = *g;
    R.G = G;
    amc_sample_blocks_config(c, "AMC_CORR_BLOCKS", &R.blocks_env, &R.max_blocks);
    R.stride = (std::max<int64_t>(c->n, 1) + 1) & ~(int64_t)1;
    const size_t M = (size_t)G.bins * AMC_CORR_Q;
    if (dalloc(c, &R.slab, (size_t)R.max_blocks * (2 * M + 1)) != hipSuccess || dalloc(c, &R.tot, corr_totals(R).words) != hipSuccess ||
        dalloc(c, &R.meta, 4) != hipSuccess || dalloc(c, &R.origin, (size_t)6 * (size_t)R.stride) != hipSuccess) {
        corr_free(c);
        return amc_fail(c, AMC_ERR_HIP, "amc_corr_config: device allocation failed");
    }
    R.on = true;
    int rc = AMC_OK;
    if (hipMemsetAsync(R.origin, 0, sizeof(double) * 6 * (size_t)R.stride, c->stream) != hipSuccess) rc = amc_fail(c, AMC_ERR_HIP, "amc_corr_config: hipMemsetAsync failed");
    if (!rc) rc = amc_corr_reset(c);
    if (rc) { corr_free(c); return rc; }
    return AMC_OK;
}

int amc_corr_sample(amc_ctx *c)
{
    if (!c) return AMC_ERR_INVALID;
    if (int rc = amc_sampler_sample_ready(c, c->CR.on, "amc_corr")) return rc;
    return corr_enqueue(c);
}

int amc_corr_read(amc_ctx *c, int64_t *totals, int64_t *n_origins, int64_t *n_samples, int64_t *n_outside, int64_t *window_pos)
{
    if (!c) return AMC_ERR_INVALID;
    if (int rc = amc_sampler_ready(c, c->CR.on, "amc_corr", "read")) return rc;
    amc_corr_ws &R = c->CR;
    unsigned long long meta[4], bad;
    if (int rc = amc_totals_get(c, corr_totals(R), totals, meta, &bad)) return rc;
    if (bad != ~0ULL)
        return amc_fail(c, AMC_ERR_CAPACITY, "amc_corr: particle %llu is outside the quantisers' range (a displacement component of 2^-18 m or more "
                        "from its origin, a velocity component of 2^14 m/s or more, or NaN); sampling stopped until amc_corr_reset", bad);
    if (n_origins) *n_origins = (int64_t)meta[0];
    if (n_samples) *n_samples = (int64_t)meta[1];
    if (n_outside) *n_outside = (int64_t)meta[2];
    if (window_pos) *window_pos = R.pos;
    return AMC_OK;
}

int amc_corr_origin(amc_ctx *c, double *x0, double *y0, double *z0, double *vx0, double *vy0, double *vz0)
{
    if (!c) return AMC_ERR_INVALID;
    if (int rc = amc_sampler_ready(c, c->CR.on, "amc_corr", "origin")) return rc;
    amc_corr_ws &R = c->CR;
    double *dst[6] = {x0, y0, z0, vx0, vy0, vz0};
    const size_t bytes = sizeof(double) * (size_t)(c->hi - c->lo);
    for (int k = 0; k < 6; k++)
        if (dst[k] && bytes) AMC_HIP(c, hipMemcpyAsync(dst[k], R.origin + (size_t)k * (size_t)R.stride + c->lo, bytes, hipMemcpyDeviceToHost, c->stream));
    AMC_HIP(c, hipStreamSynchronize(c->stream));
    return AMC_OK;
}

int amc_corr_load(amc_ctx *c, const int64_t *totals, int64_t n_origins, int64_t n_samples, int64_t n_outside, int64_t window_pos,
                  const double *x0, const double *y0, const double *z0, const double *vx0, const double *vy0, const double *vz0)
{
    if (!c || !totals || n_origins < 0 || n_samples < 0 || n_outside < 0) return AMC_ERR_INVALID;
    if (!c->CR.on) return amc_fail(c, AMC_ERR_STATE, "amc_corr_load before amc_corr_config");
    amc_corr_ws &R = c->CR;
    const double *src[6] = {x0, y0, z0, vx0, vy0, vz0};
    if (window_pos < 0 || window_pos > R.g.n_lags)
        return amc_fail(c, AMC_ERR_INVALID, "amc_corr_load: window position %lld (0 .. n_lags = %d)", (long long)window_pos, R.g.n_lags);
    for (int k = 0; k < 6; k++)
        if (window_pos > 0 && !src[k]) return amc_fail(c, AMC_ERR_INVALID, "amc_corr_load: a window position > 0 needs the six origin arrays");
    AMC_HIP(c, hipSetDevice(c->device));
    const unsigned long long meta[4] = {(unsigned long long)n_origins, (unsigned long long)n_samples, (unsigned long long)n_outside, 0};
    if (int rc = amc_totals_put(c, corr_totals(R), totals, meta)) return rc;
    const size_t bytes = sizeof(double) * (size_t)(c->hi - c->lo);
    for (int k = 0; k < 6; k++)
        if (src[k] && bytes) AMC_HIP(c, hipMemcpyAsync(R.origin + (size_t)k * (size_t)R.stride + c->lo, src[k], bytes, hipMemcpyHostToDevice, c->stream));
    AMC_HIP(c, hipStreamSynchronize(c->stream));
    R.pos = window_pos;
    return AMC_OK;
}

int amc_corr_reset(amc_ctx *c)
{
    if (!c) return AMC_ERR_INVALID;
    if (int rc = amc_sampler_ready(c, c->CR.on, "amc_corr", "reset")) return rc;
    const unsigned long long meta[4] = {0, 0, 0, 0};
    if (int rc = amc_totals_put(c, corr_totals(c->CR), nullptr, meta)) return rc;
    c->CR.pos = 0;
    return AMC_OK;
}

}  // extern "C"
