// amc_vdf.hip — sampled velocity distributions: per region of a spatial grid, histograms of the three velocity components and
// of the speed, accumulated as exact integer counts (include/argonmc_vdf.h).  The reference has no such output; the
// Python layer derives probability densities and the Maxwell comparison from the totals.
//
// One sample is two kernels, the streaming samplers' pair (amc_sample_dev.h):
//   k_vdf_accum    a persistent grid of at most one workgroup per CU.  Each workgroup streams a contiguous index range (x, y, z,
//                  vx, vy, vz: 48 B per particle, 16-B loads of particle pairs), computes the region, the components and the
//                  speed of each particle and adds one into five columns of a table of 32-bit counters in LDS (LDS atomics whose
//                  result nobody reads: exact and order-free).  It stores the table as one slab row [regions * C][outside] with
//                  plain stores — no global atomics but the atomicMin on the error word.
//   k_slab_reduce<unsigned int, vdf_sink>  sums the slab rows per column; the sink adds the result into the 64-bit running
//                  totals, and nothing once the error word is set.
// Integer sums do not depend on the order of the adds, so the totals are bitwise the same for any number of workgroups.
#include "amc_host.h"
#include "amc_sample_dev.h"

#define AMC_VDF_THREADS 1024            // the 96 KiB table leaves room for one workgroup per CU: 16 waves
// Why 32-bit counters are exact: amc_sample_blocks refuses a sample of more than AMC_SAMPLE_MAX_PARTICLES = 2^24 particles, a
// workgroup sees a part of them, and a particle adds 1 to any one column at most once (count, one column of each component's
// histogram, one of the speed's: five different columns).  So no counter of a table, nor a workgroup's count of particles
// outside, exceeds 2^24 — and the sum of one column over all slab rows is at most 2^24 too.
static_assert(AMC_SAMPLE_MAX_PARTICLES < (1LL << 32), "one sample's counts fit the table's 32-bit counters");
static_assert(AMC_VDF_MAX_COLUMNS * sizeof(unsigned int) == 96 * 1024, "the table is 96 KiB of LDS: one workgroup per CU");
static_assert(4 * AMC_VDF_MAX_HIST_BINS + 8 <= AMC_VDF_MAX_COLUMNS, "one region of the longest histograms fits the table");

// the grid as the kernel takes it
struct amc_vdf_dev {
    amc_fields_grid_dev G;
    int H, C;                           // bins per histogram, columns per region: 4 * H + 8
    double v_max, wc, ws;               // wc = 2 * v_max / H, ws = v_max / H
};

AMC_DEV void vdf_count(unsigned int *p) { (void)__hip_atomic_fetch_add(p, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// one particle into the workgroup's table; returns false if a component is out of the samplers' range
AMC_DEV bool vdf_particle(const amc_vdf_dev &V, unsigned int *tab, unsigned int &outside, double x, double y, double z, double vx,
                          double vy, double vz)
{
    int bin;
    double c[3];
    if (!amc_sample_frame(V.G, x, y, z, vx, vy, vz, bin, c)) { outside++; return true; }
    if (!amc_sample_speed_ok(c[0], c[1], c[2])) return false;
    unsigned int *a = tab + bin * V.C;
    const int H = V.H;
    vdf_count(a);
#pragma unroll
    for (int e = 0; e < 3; e++) {       // under, h[0..H), over
        const int k = amc_fields_axis(c[e], -V.v_max, V.v_max, V.wc, H);
        vdf_count(a + 1 + e * (H + 2) + (k >= 0 ? 1 + k : c[e] < -V.v_max ? 0 : H + 1));
    }
    const double s = sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
    const int k = amc_fields_axis(s, 0.0, V.v_max, V.ws, H);
    vdf_count(a + 1 + 3 * (H + 2) + (k >= 0 ? k : H));      // h[0..H), over
    return true;
}

__global__ __launch_bounds__(AMC_VDF_THREADS) void k_vdf_accum(amc_state S, amc_lazy L, long long lo, long long hi, amc_vdf_dev V,
                                                               unsigned int *slab, unsigned long long *bad)
{
    __shared__ unsigned int tab[AMC_VDF_MAX_COLUMNS];   // G.bins * C counters (the sampler's column limit)
    __shared__ unsigned int outside_sum;
    const int M = V.G.bins * V.C;
    amc_slab_begin(tab, M, &outside_sum);
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
            if (!vdf_particle(V, tab, outside, x[e], y[e], z[e], vx[e], vy[e], vz[e]) && first_bad < 0) first_bad = p;
        }
    }
    if (outside) atomicAdd(&outside_sum, outside);
    if (first_bad >= 0) atomicMin(bad, (unsigned long long)first_bad);
    amc_slab_store(slab, tab, M, &outside_sum);
}

// the distributions' end of k_slab_reduce: column j is the totals' (region, column) j; a sum is at most 2^24, one sample's particles
// meta: [0] unused, [1] samples, [2] particles outside, [3] lowest particle out of range (~0: none)
struct vdf_sink {
    static constexpr bool companion = false;
    unsigned long long *tot, *meta;
    AMC_DEV bool stopped() const { return amc_g(meta)[3] != ~0ULL; }    // a sample with a particle out of range adds nothing, nor does a later one
    AMC_DEV int stride(int W) const { return W + 1; }
    AMC_DEV void column(int j, unsigned long long s) const { amc_g(tot)[j] += s; }
    AMC_DEV void counters(unsigned long long s) const { amc_g(meta)[1] += 1; amc_g(meta)[2] += s; }
};

// ---- the host side -------------------------------------------------------------------------------------------------------------
int amc_vdf_enqueue(amc_ctx *c)        // (AMC_INTERNAL: the cadence hook's)
{
    amc_vdf_ws &F = c->VD;
    int blocks;
    if (int rc = amc_sample_blocks(c, "amc_vdf", F.blocks_env, F.max_blocks, &blocks)) return rc;
    amc_vdf_dev V;
    V.G = F.G; V.H = F.g.hist_bins; V.C = F.C; V.v_max = F.g.v_max; V.wc = F.wc; V.ws = F.ws;
    const int W = F.G.bins * F.C;
    amc_prof_begin(c, AMC_K_FIELDS);
    AMC_LAUNCH(c, k_vdf_accum, dim3(blocks), dim3(AMC_VDF_THREADS), c->S, amc_sample_lazy(c), (long long)c->lo, (long long)c->hi, V, F.slab,
               F.meta + 3);
    amc_prof_end(c);
    AMC_HIP(c, hipGetLastError());
    AMC_HIP(c, amc_launch_slab_reduce(c, (const unsigned int *)F.slab, blocks, W, vdf_sink{F.tot, F.meta}));
    return AMC_OK;
}

static void vdf_free(amc_ctx *c)
{
    ctx_free(c, c->VD.slab, c->VD.tot, c->VD.meta);
    c->VD = amc_vdf_ws();
}

static amc_totals vdf_totals(const amc_vdf_ws &F) { return amc_totals{F.tot, (size_t)F.G.bins * (size_t)F.C, F.meta, 4, 3}; }

extern "C" {

int amc_vdf_reset(amc_ctx *c) { return c ? amc_sampler_reset(c, c->VD.on, "amc_vdf", vdf_totals(c->VD)) : AMC_ERR_INVALID; }

int amc_vdf_config(amc_ctx *c, const amc_vdf_grid *g)
{
    bool done;
    if (int rc = amc_sampler_config_begin(c, g, "amc_vdf_grid", vdf_free, &done); rc || done) return rc;
    const char *fault = nullptr;
    if (g->hist_bins < 1 || g->hist_bins > AMC_VDF_MAX_HIST_BINS) fault = "hist_bins must be 1 .. 256";
    else if (!(isfinite(g->v_max) && g->v_max > 0.0 && g->v_max <= 16384.0)) fault = "v_max must be finite, > 0 and at most 16384 m/s";
    const int C = 4 * (g->hist_bins >= 1 && g->hist_bins <= AMC_VDF_MAX_HIST_BINS ? g->hist_bins : 1) + 8;
    amc_fields_grid_dev G;
    if (int rc = amc_sample_grid_check(c, "amc_vdf_grid", "regions (4 * hist_bins + 8 columns each, 24,576 columns in all)", g->kind, g->n1, g->n2,
                                       g->n3, AMC_VDF_MAX_COLUMNS / C, g->lo, g->hi, g->every, g->step_offset,
                                       g->reserved[0] == 0 && g->reserved[1] == 0, fault, &G))
        return rc;
    vdf_free(c);
    amc_vdf_ws &F = c->VD;
    F.g = *g;
    F.G = G;
    F.C = C;
    F.wc = 2.0 * g->v_max / (double)g->hist_bins;
    F.ws = g->v_max / (double)g->hist_bins;
    amc_sample_blocks_config(c, "AMC_VDF_BLOCKS", &F.blocks_env, &F.max_blocks);
    if (dalloc(c, &F.slab, (size_t)F.max_blocks * ((size_t)G.bins * C + 1)) != hipSuccess || dalloc(c, &F.tot, vdf_totals(F).words) != hipSuccess ||
        dalloc(c, &F.meta, 4) != hipSuccess) {
        vdf_free(c);
        return amc_fail(c, AMC_ERR_HIP, "amc_vdf_config: device allocation failed");
    }
    F.on = true;
    if (int rc = amc_vdf_reset(c)) { vdf_free(c); return rc; }
    return AMC_OK;
}

int amc_vdf_sample(amc_ctx *c) { return c ? amc_sampler_sample(c, c->VD.on, "amc_vdf", amc_vdf_enqueue) : AMC_ERR_INVALID; }

int amc_vdf_read(amc_ctx *c, int64_t *totals, int64_t *n_samples, int64_t *n_outside)
{ return c ? amc_sampler_read(c, c->VD.on, "amc_vdf", vdf_totals(c->VD), totals, n_samples, n_outside) : AMC_ERR_INVALID; }

int amc_vdf_load(amc_ctx *c, const int64_t *totals, int64_t n_samples, int64_t n_outside)
{ return c ? amc_sampler_load(c, c->VD.on, "amc_vdf", vdf_totals(c->VD), totals, n_samples, n_outside) : AMC_ERR_INVALID; }

}  // extern "C"
