// amc_vdf.hip — sampled velocity distributions: per region of a spatial grid, histograms of the three velocity components and
// of the speed, accumulated as exact integer counts (include/argonmc_vdf.h).  The reference has no such output; the
// Python layer derives probability densities and the Maxwell comparison from the totals.
//
// One sample is two kernels, the shape of the moment samplers' (amc_fields.hip):
//   k_vdf_accum    a persistent grid of at most one workgroup per CU.  Each workgroup streams a contiguous index range (x, y, z,
//                  vx, vy, vz: 48 B per particle, 16-B loads of particle pairs), computes the region, the components and the
//                  speed of each particle and adds one into five columns of a table of 32-bit counters in LDS (LDS atomics whose
//                  result nobody reads: exact and order-free).  It stores the table as one slab row [regions * C][outside] with
//                  plain stores — no global atomics but the atomicMin on the error word.
//   k_vdf_reduce   sums the slab rows per column and adds the result into the 64-bit running totals; it adds nothing once the
//                  error word is set.
// Integer sums do not depend on the order of the adds, so the totals are bitwise the same for any number of workgroups.
#include "amc_host.h"
#include "amc_sample_dev.h"

#define AMC_VDF_THREADS 1024            // the 96 KiB table leaves room for one workgroup per CU: 16 waves
#define AMC_VDF_REDUCE_THREADS 1024
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

// an aligned pair of particles' values: one 16-byte load from device memory
AMC_DEV double2 vdf_pair(const double *p) { return amc_g_load((const double2 *)p); }
AMC_DEV void vdf_count(unsigned int *p) { (void)__hip_atomic_fetch_add(p, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// one particle into the workgroup's table; returns false if a component is out of the samplers' range.  (Region and components
// are amc_sample_bin's and the fields' rule written out, as in amc_moments_particle.)
AMC_DEV bool vdf_particle(const amc_vdf_dev &V, unsigned int *tab, unsigned int &outside, double x, double y, double z, double vx,
                          double vy, double vz)
{
    const amc_fields_grid_dev &G = V.G;
    int i1, i2, i3;
    double c[3];
    if (G.kind == AMC_FIELDS_CARTESIAN) {
        i1 = amc_fields_axis(x, G.lo[0], G.hi[0], G.w[0], G.n1);
        i2 = amc_fields_axis(y, G.lo[1], G.hi[1], G.w[1], G.n2);
        i3 = amc_fields_axis(z, G.lo[2], G.hi[2], G.w[2], G.n3);
        c[0] = vx; c[1] = vy; c[2] = vz;
    } else {
        const double r = sqrt(x * x + y * y);
        i1 = amc_fields_axis(r, G.lo[0], G.hi[0], G.w[0], G.n1);
        i2 = amc_fields_axis(z, G.lo[1], G.hi[1], G.w[1], G.n2);
        i3 = 0;
        if (r > 0.0) {
            c[0] = (x * vx + y * vy) / r;
            c[1] = (x * vy - y * vx) / r;
        } else {
            c[0] = vx; c[1] = vy;
        }
        c[2] = vz;
    }
    if (i1 < 0 || i2 < 0 || i3 < 0) { outside++; return true; }
    if (!amc_sample_speed_ok(c[0], c[1], c[2])) return false;
    unsigned int *a = tab + ((i1 * G.n2 + i2) * G.n3 + i3) * V.C;
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
    for (int j = threadIdx.x; j < M; j += blockDim.x) tab[j] = 0;
    if (threadIdx.x == 0) outside_sum = 0;
    __syncthreads();
    const auto *gx = amc_g(S.x), *gy = amc_g(S.y), *gz = amc_g(S.z), *gvx = amc_g(S.vx), *gvy = amc_g(S.vy), *gvz = amc_g(S.vz);
    // this workgroup's particles [b0, b1), walked as aligned pairs (2k, 2k + 1): one 16-byte load per array and pair
    const long long cnt = hi - lo;
    const long long per = (cnt + gridDim.x - 1) / gridDim.x;
    const long long b0 = lo + per * blockIdx.x, b1 = b0 + per < hi ? b0 + per : hi;
    unsigned int outside = 0;
    long long first_bad = -1;
    if (b0 < b1) {
        for (long long k = (b0 >> 1) + threadIdx.x; 2 * k < b1; k += blockDim.x) {
            const long long p0 = 2 * k, p1 = p0 + 1;
            const bool v0 = p0 >= b0, v1 = p1 < b1;
            double x[2], y[2], z[2], vx[2], vy[2], vz[2];
            if (v0 && v1) {
                const double2 ax = vdf_pair(S.x + p0), ay = vdf_pair(S.y + p0), az = vdf_pair(S.z + p0);
                const double2 bx = vdf_pair(S.vx + p0), by = vdf_pair(S.vy + p0), bz = vdf_pair(S.vz + p0);
                x[0] = ax.x; x[1] = ax.y; y[0] = ay.x; y[1] = ay.y; z[0] = az.x; z[1] = az.y;
                vx[0] = bx.x; vx[1] = bx.y; vy[0] = by.x; vy[1] = by.y; vz[0] = bz.x; vz[1] = bz.y;
            } else {
                const long long p = v0 ? p0 : p1;
                const int e = v0 ? 0 : 1;
                x[e] = gx[p]; y[e] = gy[p]; z[e] = gz[p]; vx[e] = gvx[p]; vy[e] = gvy[p]; vz[e] = gvz[p];
            }
            for (int e = 0; e < 2; e++) {
                if (!(e == 0 ? v0 : v1)) continue;
                const long long p = p0 + e;
                amc_fields_lazy(S, L, p, x[e], y[e], z[e], vx[e], vy[e], vz[e]);
                if (!vdf_particle(V, tab, outside, x[e], y[e], z[e], vx[e], vy[e], vz[e]) && first_bad < 0) first_bad = p;
            }
        }
    }
    if (outside) atomicAdd(&outside_sum, outside);
    if (first_bad >= 0) atomicMin(bad, (unsigned long long)first_bad);
    __syncthreads();
    auto *row = amc_g(slab) + (size_t)blockIdx.x * (size_t)(M + 1);
    for (int j = threadIdx.x; j < M; j += blockDim.x) row[j] = tab[j];
    if (threadIdx.x == 0) row[M] = outside_sum;
}

// column j of the slab (j < W: (region, column) of the totals; j == W: particles outside) summed over the rows -> running totals.
// The geometry of k_sample_reduce: 64 columns per workgroup, its sixteen waves take every sixteenth row.
// meta: [0] unused, [1] samples, [2] particles outside, [3] lowest particle out of range (~0: none)
__global__ __launch_bounds__(AMC_VDF_REDUCE_THREADS) void k_vdf_reduce(const unsigned int *slab, int rows, int W, unsigned long long *tot,
                                                                       unsigned long long *meta)
{
    if (*amc_g(meta + 3) != ~0ULL) return;      // a sample with a particle out of range adds nothing, nor does a later one (the read reports it)
    constexpr int WAVES = AMC_VDF_REDUCE_THREADS / 64;
    __shared__ unsigned long long part[WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + lane;
    unsigned long long s = 0;           // (at most 2^24: one sample's particles)
    if (j <= W) {
        const auto *col = amc_g(slab) + j;
#pragma unroll 4
        for (int b = wave; b < rows; b += WAVES) s += col[(size_t)b * (size_t)(W + 1)];
    }
    part[wave][lane] = s;
    __syncthreads();
    if (wave != 0 || j > W) return;
    s = 0;
#pragma unroll
    for (int k = 0; k < WAVES; k++) s += part[k][lane];
    if (j == W) {
        amc_g(meta)[1] += 1;
        amc_g(meta)[2] += s;
        return;
    }
    amc_g(tot)[j] += s;
}

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
    amc_prof_begin(c, AMC_K_FIELDS);
    AMC_LAUNCH(c, k_vdf_reduce, dim3((W + 1 + 63) / 64), dim3(AMC_VDF_REDUCE_THREADS), (const unsigned int *)F.slab, blocks, W, F.tot, F.meta);
    amc_prof_end(c);
    AMC_HIP(c, hipGetLastError());
    return AMC_OK;
}

static void vdf_free(amc_ctx *c)
{
    ctx_free(c, c->VD.slab, c->VD.tot, c->VD.meta);
    c->VD = amc_vdf_ws();
}

static amc_totals vdf_totals(const amc_vdf_ws &F) { return amc_totals{F.tot, (size_t)F.G.bins * (size_t)F.C, F.meta, 4, 3}; }

extern "C" {

int amc_vdf_reset(amc_ctx *c)
{
    if (!c) return AMC_ERR_INVALID;
    if (int rc = amc_sampler_ready(c, c->VD.on, "amc_vdf", "reset")) return rc;
    const unsigned long long meta[4] = {0, 0, 0, 0};
    return amc_totals_put(c, vdf_totals(c->VD), nullptr, meta);
}

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

int amc_vdf_sample(amc_ctx *c)
{
    if (!c) return AMC_ERR_INVALID;
    if (int rc = amc_sampler_sample_ready(c, c->VD.on, "amc_vdf")) return rc;
    return amc_vdf_enqueue(c);
}

int amc_vdf_read(amc_ctx *c, int64_t *totals, int64_t *n_samples, int64_t *n_outside)
{
    if (!c) return AMC_ERR_INVALID;
    if (int rc = amc_sampler_ready(c, c->VD.on, "amc_vdf", "read")) return rc;
    unsigned long long meta[4], bad;
    if (int rc = amc_totals_get(c, vdf_totals(c->VD), totals, meta, &bad)) return rc;
    if (bad != ~0ULL)
        return amc_fail(c, AMC_ERR_CAPACITY, "amc_vdf: particle %llu has a velocity component outside |c| < 2^14 m/s (or NaN); "
                        "sampling stopped until amc_vdf_reset", bad);
    if (n_samples) *n_samples = (int64_t)meta[1];
    if (n_outside) *n_outside = (int64_t)meta[2];
    return AMC_OK;
}

int amc_vdf_load(amc_ctx *c, const int64_t *totals, int64_t n_samples, int64_t n_outside)
{
    if (!c || !totals || n_samples < 0 || n_outside < 0) return AMC_ERR_INVALID;
    if (int rc = amc_sampler_ready(c, c->VD.on, "amc_vdf", "load")) return rc;
    const unsigned long long meta[4] = {0, (unsigned long long)n_samples, (unsigned long long)n_outside, 0};
    return amc_totals_put(c, vdf_totals(c->VD), totals, meta);
}

}  // extern "C"
