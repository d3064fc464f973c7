// amc_fields.hip — the moment samplers.  Sampled fields: per spatial bin, the particle count and the first and second moments
// of the velocity components, accumulated as exact integers (include/argonmc.h "sampled fields").  Sampled
// fluxes: the same seven (row A) and a second row B of the three cross products and the three energy-weighted components
// (include/argonmc_flux.h).  The reference has neither output; the Python layer derives number density, flow
// velocity and temperature, the pressure tensor, the energy flux and the heat flux from the totals.
//
// One sample is two kernels:
//   k_moments_accum<ROWS>  (ROWS = 1: the fields, 2: the fluxes) a persistent grid of at most one workgroup per CU.  Each
//                    workgroup streams a contiguous index range (x, y, z, vx, vy, vz: 48 B per particle, 16-B loads of
//                    particle pairs), computes the bin and the seven or thirteen non-zero integers of each particle and adds
//                    them into ROWS tables in LDS (64-bit integer LDS atomics: exact and order-free).  It stores the tables
//                    as one slab row [ROWS][bins * 7][outside] with plain stores — no global atomics but the atomicMin on
//                    the error word.
//   k_slab_reduce<unsigned long long, sample_sink>  (amc_sample_dev.h) sums the slab rows per (bin, quantity); the sink adds the
//                    result into the 128-bit running totals, with carry (the fluxes: row A at "lag" 0 and row B at "lag" 1 of
//                    two, totals[bins][2][7][2]); it serves the sampled correlations too (amc_launch_sample_reduce) and adds
//                    nothing once the error word is set.
// Integer sums do not depend on the order of the adds, so the totals are bitwise the same for any number of workgroups.
#include "amc_host.h"
#include "amc_sample_dev.h"
#include <cstddef>

#define AMC_MOMENTS_Q AMC_SAMPLE_Q       // per row — A: count, q1(c1..c3), q2(c1..c3); B: 0, q2(c1c2, c1c3, c2c3), q3(c1..c3)
#define AMC_MOMENTS_THREADS 1024        // the 112 KiB of tables leave room for one workgroup per CU: 16 waves
static_assert(2 * AMC_FLUX_MAX_BINS == AMC_FIELDS_MAX_BINS, "both instances of k_moments_accum fill the one LDS table");

AMC_DEV unsigned long long moments_q1(double c) { return (unsigned long long)(long long)rint(c * 16777216.0); }
AMC_DEV unsigned long long moments_q2(double a, double b) { return (unsigned long long)(long long)rint((a * b) * 1024.0); }
AMC_DEV unsigned long long moments_q3(double e, double c) { return (unsigned long long)(long long)rint(ldexp(e * c, -6)); }

// one particle into the workgroup's tables (tab: row A; ROWS == 2: tab + M is row B); returns false if a component is out of
// the quantisation range
template <int ROWS>
AMC_DEV bool amc_moments_particle(const amc_fields_grid_dev &G, unsigned long long *tab, int M, unsigned int &outside, double x, double y,
                                  double z, double vx, double vy, double vz)
{
    int bin;
    double c[3];
    if (!amc_sample_frame(G, x, y, z, vx, vy, vz, bin, c)) { outside++; return true; }
    const double c1 = c[0], c2 = c[1], c3 = c[2];
    if (!amc_sample_speed_ok(c1, c2, c3)) return false;
    unsigned long long *a = tab + (size_t)bin * AMC_MOMENTS_Q;
    const double s1 = c1 * c1, s2 = c2 * c2, s3 = c3 * c3;
    atomicAdd(a + 0, 1ULL);
    atomicAdd(a + 1, moments_q1(c1));
    atomicAdd(a + 2, moments_q1(c2));
    atomicAdd(a + 3, moments_q1(c3));
    atomicAdd(a + 4, (unsigned long long)(long long)rint(s1 * 1024.0));
    atomicAdd(a + 5, (unsigned long long)(long long)rint(s2 * 1024.0));
    atomicAdd(a + 6, (unsigned long long)(long long)rint(s3 * 1024.0));
    if constexpr (ROWS == 2) {
        unsigned long long *b = a + M;
        const double e = (s1 + s2) + s3;
        atomicAdd(b + 1, moments_q2(c1, c2));
        atomicAdd(b + 2, moments_q2(c1, c3));
        atomicAdd(b + 3, moments_q2(c2, c3));
        atomicAdd(b + 4, moments_q3(e, c1));
        atomicAdd(b + 5, moments_q3(e, c2));
        atomicAdd(b + 6, moments_q3(e, c3));
    }
    return true;
}

template <int ROWS>
__global__ __launch_bounds__(AMC_MOMENTS_THREADS) void k_moments_accum(amc_state S, amc_lazy L, long long lo, long long hi,
                                                                       amc_fields_grid_dev G, unsigned long long *slab,
                                                                       unsigned long long *bad)
{
    __shared__ unsigned long long tab[AMC_FIELDS_MAX_BINS * AMC_MOMENTS_Q];     // ROWS tables of G.bins * 7 (the sampler's bin limit)
    __shared__ unsigned int outside_sum;
    const int M = G.bins * AMC_MOMENTS_Q;
    amc_slab_begin(tab, ROWS * M, &outside_sum);
    unsigned int outside = 0;
    long long first_bad = -1;
    for (amc_sample_walk w(lo, hi); w.more(); w.next()) {
        const long long p0 = w.p0();
        const bool v0 = w.v0(), v1 = w.v1();
        double x[2], y[2], z[2], vx[2], vy[2], vz[2];
        amc_sample_load_pair(S, p0, v0, v1, x, y, z, vx, vy, vz);
        for (int e = 0; e < 2; e++) {
            if (!(e == 0 ? v0 : v1)) continue;
            const long long p = p0 + e;
            amc_fields_lazy(L, p, x[e], y[e], z[e], vx[e], vy[e], vz[e]);
            if (!amc_moments_particle<ROWS>(G, tab, M, outside, x[e], y[e], z[e], vx[e], vy[e], vz[e]) && first_bad < 0) first_bad = p;
        }
    }
    if (outside) atomicAdd(&outside_sum, outside);
    if (first_bad >= 0) atomicMin(bad, (unsigned long long)first_bad);
    amc_slab_store(slab, tab, ROWS * M, &outside_sum);
}

// The moment samplers' and the correlations' end of k_slab_reduce: column j of the slab is table j / M, (bin, quantity) j % M, and
// goes with carry into the 128-bit running totals at lag_a (table 0) or lag_b (table 1) of lags1.
// meta: [0] origins, [1] samples, [2] particles outside, [3] lowest particle out of range (~0: none)
struct sample_sink {
    static constexpr bool companion = false;
    int M, lag_a, lag_b, lags1, origin;
    unsigned long long *tot, *meta;
    AMC_DEV bool stopped() const { return amc_g(meta)[3] != ~0ULL; }    // a sample with a particle out of range adds nothing, nor does a later one
    AMC_DEV int stride(int W) const { return W + 1; }
    AMC_DEV void column(int j, unsigned long long s) const       // (the true sum of one sample is below 2^62 in magnitude)
    {
        const int t = j / M, jj = j - t * M;
        const int g = jj / AMC_SAMPLE_Q, q = jj - g * AMC_SAMPLE_Q;
        auto *at = amc_g(tot) + 2 * (((size_t)g * (size_t)lags1 + (size_t)(t == 0 ? lag_a : lag_b)) * AMC_SAMPLE_Q + (size_t)q);
        unsigned long long tl = at[0], th = at[1];
        amc_add128(tl, th, s);
        at[0] = tl; at[1] = th;
    }
    AMC_DEV void counters(unsigned long long s) const
    {
        amc_g(meta)[0] += (unsigned long long)origin;
        amc_g(meta)[1] += 1;
        amc_g(meta)[2] += s;
    }
};

hipError_t amc_launch_sample_reduce(amc_ctx *c, const unsigned long long *slab, int rows, int M, int tables, int lag_a, int lag_b,
                                    int lags1, int origin, unsigned long long *tot, unsigned long long *meta)
{
    return amc_launch_slab_reduce(c, slab, rows, tables * M, sample_sink{M, lag_a, lag_b, lags1, origin, tot, meta});
}

// ---- the host side: one implementation over a workspace (c->F, c->FX) and its sampler's descriptor -------------------------------------------
struct moments_desc {
    const char *name, *grid;            // in the messages: the entry points' prefix and the grid struct
    const char *env;                    // the workgroups' environment knob
    int max_bins, rows;
};
static const moments_desc FIELDS = {"amc_fields", "amc_field_grid", "AMC_FIELDS_BLOCKS", AMC_FIELDS_MAX_BINS, 1};
static const moments_desc FLUX = {"amc_flux", "amc_flux_grid", "AMC_FLUX_BLOCKS", AMC_FLUX_MAX_BINS, 2};

// amc_flux_grid is amc_field_grid member for member: the workspace stores either as the latter
#define MOMENTS_SAME(m) static_assert(offsetof(amc_flux_grid, m) == offsetof(amc_field_grid, m) && \
                                      sizeof(amc_flux_grid::m) == sizeof(amc_field_grid::m), "amc_flux_grid." #m " differs from amc_field_grid's")
static_assert(sizeof(amc_flux_grid) == sizeof(amc_field_grid), "amc_flux_grid differs in size from amc_field_grid");
MOMENTS_SAME(struct_size); MOMENTS_SAME(kind); MOMENTS_SAME(n1); MOMENTS_SAME(n2); MOMENTS_SAME(n3); MOMENTS_SAME(reserved);
MOMENTS_SAME(every); MOMENTS_SAME(step_offset); MOMENTS_SAME(lo); MOMENTS_SAME(hi);
#undef MOMENTS_SAME

static int moments_enqueue(amc_ctx *c, amc_moments_ws &W, const moments_desc &D)
{
    int blocks;
    if (int rc = amc_sample_blocks(c, D.name, W.blocks_env, W.max_blocks, &blocks)) return rc;
    amc_prof_begin(c, AMC_K_FIELDS);
    if (D.rows == 1)
        AMC_LAUNCH(c, k_moments_accum<1>, dim3(blocks), dim3(AMC_MOMENTS_THREADS), c->S, amc_sample_lazy(c), (long long)c->lo, (long long)c->hi,
                   W.G, W.slab, W.meta + 3);
    else
        AMC_LAUNCH(c, k_moments_accum<2>, dim3(blocks), dim3(AMC_MOMENTS_THREADS), c->S, amc_sample_lazy(c), (long long)c->lo, (long long)c->hi,
                   W.G, W.slab, W.meta + 3);
    amc_prof_end(c);
    AMC_HIP(c, hipGetLastError());
    // row A is table 0 -> totals[bin][0], row B table 1 -> totals[bin][1]
    AMC_HIP(c, amc_launch_sample_reduce(c, W.slab, blocks, W.G.bins * AMC_MOMENTS_Q, D.rows, 0, D.rows - 1, D.rows, 0, W.tot, W.meta));
    return AMC_OK;
}

static void moments_free(amc_ctx *c, amc_moments_ws &W)
{
    ctx_free(c, W.slab, W.tot, W.meta);
    W = amc_moments_ws();
}

// meta: [0] unused, [1] samples, [2] particles outside, [3] the error word (the layout amc_sampler_read reads)
static amc_totals moments_totals(const amc_moments_ws &W, const moments_desc &D)
{
    return amc_totals{W.tot, (size_t)2 * D.rows * AMC_MOMENTS_Q * (size_t)W.G.bins, W.meta, 4, 3};
}

// (c is not null here: the entry points have looked)
// grid: the sampler's grid struct (the common layout, above), or nullptr
static int moments_config(amc_ctx *c, amc_moments_ws &W, const moments_desc &D, const void *grid)
{
    bool done;
    if (int rc = amc_sampler_config_begin(c, (const amc_field_grid *)grid, D.grid, [&W](amc_ctx *ctx) { moments_free(ctx, W); }, &done); rc || done)
        return rc;
    amc_field_grid g;
    memcpy(&g, grid, sizeof g);
    amc_fields_grid_dev G;
    if (int rc = amc_sample_grid_check(c, D.grid, "bins", g.kind, g.n1, g.n2, g.n3, D.max_bins, g.lo, g.hi, g.every, g.step_offset,
                                       g.reserved == 0, nullptr, &G))
        return rc;
    moments_free(c, W);
    W.g = g;
    W.G = G;
    amc_sample_blocks_config(c, D.env, &W.blocks_env, &W.max_blocks);
    const size_t M = (size_t)G.bins * AMC_MOMENTS_Q;
    if (dalloc(c, &W.slab, (size_t)W.max_blocks * (D.rows * M + 1)) != hipSuccess || dalloc(c, &W.tot, moments_totals(W, D).words) != hipSuccess ||
        dalloc(c, &W.meta, 4) != hipSuccess) {
        moments_free(c, W);
        return amc_fail(c, AMC_ERR_HIP, "%s_config: device allocation failed", D.name);
    }
    W.on = true;
    if (int rc = amc_sampler_reset(c, W.on, D.name, moments_totals(W, D))) { moments_free(c, W); return rc; }
    return AMC_OK;
}

extern "C" {

int amc_fields_enqueue(amc_ctx *c) { return moments_enqueue(c, c->F, FIELDS); }
int amc_flux_enqueue(amc_ctx *c) { return moments_enqueue(c, c->FX, FLUX); }

int amc_fields_config(amc_ctx *c, const amc_field_grid *g) { return c ? moments_config(c, c->F, FIELDS, g) : AMC_ERR_INVALID; }
int amc_flux_config(amc_ctx *c, const amc_flux_grid *g) { return c ? moments_config(c, c->FX, FLUX, g) : AMC_ERR_INVALID; }

int amc_fields_sample(amc_ctx *c) { return c ? amc_sampler_sample(c, c->F.on, FIELDS.name, amc_fields_enqueue) : AMC_ERR_INVALID; }
int amc_flux_sample(amc_ctx *c) { return c ? amc_sampler_sample(c, c->FX.on, FLUX.name, amc_flux_enqueue) : AMC_ERR_INVALID; }

int amc_fields_read(amc_ctx *c, int64_t *totals, int64_t *n_samples, int64_t *n_outside)
{ return c ? amc_sampler_read(c, c->F.on, FIELDS.name, moments_totals(c->F, FIELDS), totals, n_samples, n_outside) : AMC_ERR_INVALID; }
int amc_flux_read(amc_ctx *c, int64_t *totals, int64_t *n_samples, int64_t *n_outside)
{ return c ? amc_sampler_read(c, c->FX.on, FLUX.name, moments_totals(c->FX, FLUX), totals, n_samples, n_outside) : AMC_ERR_INVALID; }

int amc_fields_load(amc_ctx *c, const int64_t *totals, int64_t n_samples, int64_t n_outside)
{ return c ? amc_sampler_load(c, c->F.on, FIELDS.name, moments_totals(c->F, FIELDS), totals, n_samples, n_outside) : AMC_ERR_INVALID; }
int amc_flux_load(amc_ctx *c, const int64_t *totals, int64_t n_samples, int64_t n_outside)
{ return c ? amc_sampler_load(c, c->FX.on, FLUX.name, moments_totals(c->FX, FLUX), totals, n_samples, n_outside) : AMC_ERR_INVALID; }

int amc_fields_reset(amc_ctx *c) { return c ? amc_sampler_reset(c, c->F.on, FIELDS.name, moments_totals(c->F, FIELDS)) : AMC_ERR_INVALID; }
int amc_flux_reset(amc_ctx *c) { return c ? amc_sampler_reset(c, c->FX.on, FLUX.name, moments_totals(c->FX, FLUX)) : AMC_ERR_INVALID; }

}  // extern "C"
