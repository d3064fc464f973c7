// amc_flux.hip — sampled fluxes: per spatial bin, the particle count and the first, second (all six) and contracted third
// moments of the velocity components, accumulated as exact integers (include/argonmc_flux.h).  The reference
// has no such output; the Python layer derives the pressure tensor, the energy flux and the heat flux from the totals.
//
// One sample is two kernels, shaped like the sampled fields' (amc_fields.hip):
//   k_flux_accum     a persistent grid of at most one workgroup per CU, each over a contiguous index range, 16-byte loads of
//                    particle pairs.  Per particle the bin (the fields' rule, written out as in amc_fields_particle) and the
//                    thirteen non-zero integers, added into two tables in LDS (row A: the fields' seven; row B: 0, the three
//                    cross products, the three energy-weighted components) with 64-bit integer LDS atomics.  The tables
//                    leave as one slab row [A: bins * 7][B: bins * 7][outside] with plain stores — no global atomics but the
//                    atomicMin on the error word.
//   k_sample_reduce  (amc_fields.hip) sums the slab rows per (bin, quantity) into the 128-bit totals, table 0 at "lag" 0 and
//                    table 1 at "lag" 1 of two: totals[bins][2][7][2].
// Integer sums do not depend on the order of the adds, so the totals are bitwise the same for any number of workgroups.
#include "amc_host.h"
#include "amc_sample_dev.h"

#define AMC_FLUX_Q AMC_SAMPLE_Q          // per row — A: count, q1(c1..c3), q2(c1..c3); B: 0, q2(c1c2, c1c3, c2c3), q3(c1..c3)
#define AMC_FLUX_ROWS 2
#define AMC_FLUX_THREADS 1024           // the 112 KiB of tables leave room for one workgroup per CU: 16 waves

AMC_DEV unsigned long long flux_q2(double a, double b) { return (unsigned long long)(long long)rint((a * b) * 1024.0); }
AMC_DEV unsigned long long flux_q3(double e, double c) { return (unsigned long long)(long long)rint(ldexp(e * c, -6)); }

// one particle into the workgroup's tables (tab: row A, tab + M: row B); returns false if a component is out of the
// quantisation range
AMC_DEV bool amc_flux_particle(const amc_fields_grid_dev &G, unsigned long long *tab, int M, unsigned int &outside, double x, double y,
                               double z, double vx, double vy, double vz)
{
    int i1, i2, i3;
    double c1, c2, c3;
    if (G.kind == AMC_FIELDS_CARTESIAN) {
        i1 = amc_fields_axis(x, G.lo[0], G.hi[0], G.w[0], G.n1);
        i2 = amc_fields_axis(y, G.lo[1], G.hi[1], G.w[1], G.n2);
        i3 = amc_fields_axis(z, G.lo[2], G.hi[2], G.w[2], G.n3);
        c1 = vx; c2 = vy; c3 = vz;
    } else {
        const double r = sqrt(x * x + y * y);
        i1 = amc_fields_axis(r, G.lo[0], G.hi[0], G.w[0], G.n1);
        i2 = amc_fields_axis(z, G.lo[1], G.hi[1], G.w[1], G.n2);
        i3 = 0;
        if (r > 0.0) {
            c1 = (x * vx + y * vy) / r;
            c2 = (x * vy - y * vx) / r;
        } else {
            c1 = vx; c2 = vy;
        }
        c3 = vz;
    }
    if (i1 < 0 || i2 < 0 || i3 < 0) { outside++; return true; }
    if (!amc_sample_speed_ok(c1, c2, c3)) return false;
    unsigned long long *a = tab + (size_t)((i1 * G.n2 + i2) * G.n3 + i3) * AMC_FLUX_Q, *b = a + M;
    const double s1 = c1 * c1, s2 = c2 * c2, s3 = c3 * c3;
    const double e = (s1 + s2) + s3;
    atomicAdd(a + 0, 1ULL);
    atomicAdd(a + 1, (unsigned long long)(long long)rint(c1 * 16777216.0));
    atomicAdd(a + 2, (unsigned long long)(long long)rint(c2 * 16777216.0));
    atomicAdd(a + 3, (unsigned long long)(long long)rint(c3 * 16777216.0));
    atomicAdd(a + 4, (unsigned long long)(long long)rint(s1 * 1024.0));
    atomicAdd(a + 5, (unsigned long long)(long long)rint(s2 * 1024.0));
    atomicAdd(a + 6, (unsigned long long)(long long)rint(s3 * 1024.0));
    atomicAdd(b + 1, flux_q2(c1, c2));
    atomicAdd(b + 2, flux_q2(c1, c3));
    atomicAdd(b + 3, flux_q2(c2, c3));
    atomicAdd(b + 4, flux_q3(e, c1));
    atomicAdd(b + 5, flux_q3(e, c2));
    atomicAdd(b + 6, flux_q3(e, c3));
    return true;
}

__global__ __launch_bounds__(AMC_FLUX_THREADS) void k_flux_accum(amc_state S, amc_lazy L, long long lo, long long hi, amc_fields_grid_dev G,
                                                                 unsigned long long *slab, unsigned long long *bad)
{
    __shared__ unsigned long long tab[AMC_FLUX_ROWS * AMC_FLUX_MAX_BINS * AMC_FLUX_Q];
    __shared__ unsigned int outside_sum;
    const int M = G.bins * AMC_FLUX_Q;
    for (int j = threadIdx.x; j < AMC_FLUX_ROWS * M; j += blockDim.x) tab[j] = 0;
    if (threadIdx.x == 0) outside_sum = 0;
    __syncthreads();
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
                const double2 ax = *(const double2 *)(S.x + p0), ay = *(const double2 *)(S.y + p0), az = *(const double2 *)(S.z + p0);
                const double2 bx = *(const double2 *)(S.vx + p0), by = *(const double2 *)(S.vy + p0), bz = *(const double2 *)(S.vz + p0);
                x[0] = ax.x; x[1] = ax.y; y[0] = ay.x; y[1] = ay.y; z[0] = az.x; z[1] = az.y;
                vx[0] = bx.x; vx[1] = bx.y; vy[0] = by.x; vy[1] = by.y; vz[0] = bz.x; vz[1] = bz.y;
            } else {
                const long long p = v0 ? p0 : p1;
                const int e = v0 ? 0 : 1;
                x[e] = S.x[p]; y[e] = S.y[p]; z[e] = S.z[p]; vx[e] = S.vx[p]; vy[e] = S.vy[p]; vz[e] = S.vz[p];
            }
            for (int e = 0; e < 2; e++) {
                if (!(e == 0 ? v0 : v1)) continue;
                const long long p = p0 + e;
                amc_fields_lazy(S, L, p, x[e], y[e], z[e], vx[e], vy[e], vz[e]);
                if (!amc_flux_particle(G, tab, M, outside, x[e], y[e], z[e], vx[e], vy[e], vz[e]) && first_bad < 0) first_bad = p;
            }
        }
    }
    if (outside) atomicAdd(&outside_sum, outside);
    if (first_bad >= 0) atomicMin(bad, (unsigned long long)first_bad);
    __syncthreads();
    unsigned long long *row = slab + (size_t)blockIdx.x * (size_t)(AMC_FLUX_ROWS * M + 1);
    for (int j = threadIdx.x; j < AMC_FLUX_ROWS * M; j += blockDim.x) row[j] = tab[j];
    if (threadIdx.x == 0) row[AMC_FLUX_ROWS * M] = outside_sum;
}

static int flux_enqueue(amc_ctx *c)
{
    amc_flux_ws &X = c->FX;
    int blocks;
    if (int rc = amc_sample_blocks(c, "amc_flux", X.blocks_env, X.max_blocks, &blocks)) return rc;
    amc_prof_begin(c, AMC_K_FIELDS);
    AMC_LAUNCH(c, k_flux_accum, dim3(blocks), dim3(AMC_FLUX_THREADS), c->S, amc_sample_lazy(c), (long long)c->lo, (long long)c->hi, X.G,
               X.slab, X.meta + 3);
    amc_prof_end(c);
    AMC_HIP(c, hipGetLastError());
    // row A is table 0 -> totals[bin][0], row B table 1 -> totals[bin][1]
    AMC_HIP(c, amc_launch_sample_reduce(c, X.slab, blocks, X.G.bins * AMC_FLUX_Q, AMC_FLUX_ROWS, 0, 1, AMC_FLUX_ROWS, 0, X.tot, X.meta));
    return AMC_OK;
}

static void flux_free(amc_ctx *c)
{
    ctx_free(c, c->FX.slab, c->FX.tot, c->FX.meta);
    c->FX = amc_flux_ws();
}

// meta: [0] unused, [1] samples, [2] particles outside, [3] the error word (the layout k_sample_reduce writes)
static amc_totals flux_totals(const amc_flux_ws &X)
{
    return amc_totals{X.tot, (size_t)2 * AMC_FLUX_ROWS * AMC_FLUX_Q * (size_t)X.G.bins, X.meta, 4, 3};
}

extern "C" {

int amc_flux_step(amc_ctx *c)
{
    if (!amc_flux_due(c, c->out.step)) return AMC_OK;
    return flux_enqueue(c);
}

int amc_flux_config(amc_ctx *c, const amc_flux_grid *g)
{
    if (!c) return AMC_ERR_INVALID;
    AMC_HIP(c, hipSetDevice(c->device));
    AMC_HIP(c, hipStreamSynchronize(c->stream));        // (a sample in flight may still use the old buffers)
    if (!g) {
        flux_free(c);
        return AMC_OK;
    }
    if (g->struct_size != (int32_t)sizeof(amc_flux_grid)) return amc_fail(c, AMC_ERR_INVALID, "amc_flux_grid.struct_size mismatch (ABI)");
    amc_fields_grid_dev G;
    if (int rc = amc_sample_grid_check(c, "amc_flux_grid", "bins", g->kind, g->n1, g->n2, g->n3, AMC_FLUX_MAX_BINS, g->lo, g->hi, g->every,
                                       g->step_offset, g->reserved == 0, nullptr, &G))
        return rc;
    flux_free(c);
    amc_flux_ws &X = c->FX;
    X.g = *g;
    X.G = G;
    amc_sample_blocks_config(c, "AMC_FLUX_BLOCKS", &X.blocks_env, &X.max_blocks);
    const size_t M = (size_t)G.bins * AMC_FLUX_Q;
    if (dalloc(c, &X.slab, (size_t)X.max_blocks * (AMC_FLUX_ROWS * M + 1)) != hipSuccess || dalloc(c, &X.tot, flux_totals(X).words) != hipSuccess ||
        dalloc(c, &X.meta, 4) != hipSuccess) {
        flux_free(c);
        return amc_fail(c, AMC_ERR_HIP, "amc_flux_config: device allocation failed");
    }
    X.on = true;
    if (int rc = amc_flux_reset(c)) { flux_free(c); return rc; }
    return AMC_OK;
}

int amc_flux_sample(amc_ctx *c)
{
    if (!c) return AMC_ERR_INVALID;
    if (!c->FX.on) return amc_fail(c, AMC_ERR_STATE, "amc_flux_sample before amc_flux_config");
    if (!c->uploaded) return amc_fail(c, AMC_ERR_STATE, "amc_flux_sample before amc_upload");
    AMC_HIP(c, hipSetDevice(c->device));
    return flux_enqueue(c);
}

int amc_flux_read(amc_ctx *c, int64_t *totals, int64_t *n_samples, int64_t *n_outside)
{
    if (!c) return AMC_ERR_INVALID;
    if (!c->FX.on) return amc_fail(c, AMC_ERR_STATE, "amc_flux_read before amc_flux_config");
    AMC_HIP(c, hipSetDevice(c->device));
    unsigned long long meta[4], bad;
    if (int rc = amc_totals_get(c, flux_totals(c->FX), totals, meta, &bad)) return rc;
    if (bad != ~0ULL)
        return amc_fail(c, AMC_ERR_CAPACITY, "amc_flux: particle %llu has a velocity component outside |c| < 2^14 m/s (or NaN); "
                        "sampling stopped until amc_flux_reset", bad);
    if (n_samples) *n_samples = (int64_t)meta[1];
    if (n_outside) *n_outside = (int64_t)meta[2];
    return AMC_OK;
}

int amc_flux_load(amc_ctx *c, const int64_t *totals, int64_t n_samples, int64_t n_outside)
{
    if (!c || !totals || n_samples < 0 || n_outside < 0) return AMC_ERR_INVALID;
    if (!c->FX.on) return amc_fail(c, AMC_ERR_STATE, "amc_flux_load before amc_flux_config");
    AMC_HIP(c, hipSetDevice(c->device));
    const unsigned long long meta[4] = {0, (unsigned long long)n_samples, (unsigned long long)n_outside, 0};
    return amc_totals_put(c, flux_totals(c->FX), totals, meta);
}

int amc_flux_reset(amc_ctx *c)
{
    if (!c) return AMC_ERR_INVALID;
    if (!c->FX.on) return amc_fail(c, AMC_ERR_STATE, "amc_flux_reset before amc_flux_config");
    AMC_HIP(c, hipSetDevice(c->device));
    const unsigned long long meta[4] = {0, 0, 0, 0};
    return amc_totals_put(c, flux_totals(c->FX), nullptr, meta);
}

}  // extern "C"
