// amc_fields.hip — sampled fields: per spatial bin, the particle count and the first and second moments of the velocity
// components, accumulated as exact integers (include/argonmc.h "sampled fields").  The reference has no such
// output; the Python layer derives number density, flow velocity and temperature from the totals.
//
// One sample is two kernels:
//   k_fields_accum   a persistent grid of at most one workgroup per CU.  Each workgroup streams a contiguous index range
//                    (x, y, z, vx, vy, vz: 48 B per particle, 16-B loads of particle pairs), computes the bin and the seven
//                    integers of each particle and adds them into a table in LDS (64-bit integer LDS atomics: exact and
//                    order-free).  It stores the table as one slab row with plain stores — no global atomics.
//   k_sample_reduce  sums the slab rows per (bin, quantity) and adds the result into the 128-bit running totals, with carry; it
//                    serves the sampled correlations too (amc_launch_sample_reduce) and adds nothing once the error word is set.
// Integer sums do not depend on the order of the adds, so the totals are bitwise the same for any number of workgroups.
#include "amc_host.h"
#include "amc_sample_dev.h"

#define AMC_FIELDS_Q AMC_SAMPLE_Q        // count, q1(c1..c3), q2(c1..c3)
#define AMC_FIELDS_THREADS 1024         // the 112 KiB table leaves room for one workgroup per CU: 16 waves
#define AMC_SAMPLE_REDUCE_THREADS 1024

// one particle into the workgroup's table; returns false if a component is out of the quantisation range.  (The bin is
// amc_sample_bin's rule written out: calling it here measured + 0.5 us on the cube's 16 us sample)
AMC_DEV bool amc_fields_particle(const amc_fields_grid_dev &G, unsigned long long *tab, unsigned int &outside, double x, double y,
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
    unsigned long long *t = tab + (size_t)((i1 * G.n2 + i2) * G.n3 + i3) * AMC_FIELDS_Q;
    atomicAdd(t + 0, 1ULL);
    atomicAdd(t + 1, (unsigned long long)(long long)rint(c1 * 16777216.0));
    atomicAdd(t + 2, (unsigned long long)(long long)rint(c2 * 16777216.0));
    atomicAdd(t + 3, (unsigned long long)(long long)rint(c3 * 16777216.0));
    atomicAdd(t + 4, (unsigned long long)(long long)rint((c1 * c1) * 1024.0));
    atomicAdd(t + 5, (unsigned long long)(long long)rint((c2 * c2) * 1024.0));
    atomicAdd(t + 6, (unsigned long long)(long long)rint((c3 * c3) * 1024.0));
    return true;
}

__global__ __launch_bounds__(AMC_FIELDS_THREADS) void k_fields_accum(amc_state S, amc_lazy L, long long lo, long long hi,
                                                                     amc_fields_grid_dev G, unsigned long long *slab,
                                                                     unsigned long long *bad)
{
    __shared__ unsigned long long tab[AMC_FIELDS_MAX_BINS * AMC_FIELDS_Q];
    __shared__ unsigned int outside_sum;
    const int M = G.bins * AMC_FIELDS_Q;
    for (int j = threadIdx.x; j < M; j += blockDim.x) tab[j] = 0;
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
                if (!amc_fields_particle(G, tab, outside, x[e], y[e], z[e], vx[e], vy[e], vz[e]) && first_bad < 0) first_bad = p;
            }
        }
    }
    if (outside) atomicAdd(&outside_sum, outside);
    if (first_bad >= 0) atomicMin(bad, (unsigned long long)first_bad);
    __syncthreads();
    unsigned long long *row = slab + (size_t)blockIdx.x * (size_t)(M + 1);
    for (int j = threadIdx.x; j < M; j += blockDim.x) row[j] = tab[j];
    if (threadIdx.x == 0) row[M] = outside_sum;
}

// column j of the slab (j < tables * M: table j / M, (bin, quantity) j % M; j == tables * M: particles outside) summed over
// the rows -> running totals at lag_a (table 0) or lag_b (table 1).  64 columns per workgroup, its sixteen waves take every
// sixteenth row, four loads in flight each: the rows are a chain of memory round trips otherwise (measured: 10 us for 123 rows
// with four waves).
// meta: [0] origins, [1] samples, [2] particles outside, [3] lowest particle out of range (~0: none)
__global__ __launch_bounds__(AMC_SAMPLE_REDUCE_THREADS) void k_sample_reduce(const unsigned long long *slab, int rows, int M, int tables, int lag_a,
                                                                             int lag_b, int lags1, int origin, unsigned long long *tot,
                                                                             unsigned long long *meta)
{
    if (meta[3] != ~0ULL) return;       // a sample with a particle out of range adds nothing, nor does a later one (the read reports it)
    constexpr int WAVES = AMC_SAMPLE_REDUCE_THREADS / 64;
    __shared__ unsigned long long part[WAVES][64];
    const int W = tables * M;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + lane;
    unsigned long long s = 0;           // (wraps modulo 2^64; the true sum of one sample is below 2^62 in magnitude)
    if (j <= W) {
#pragma unroll 4
        for (int b = wave; b < rows; b += WAVES) s += slab[(size_t)b * (size_t)(W + 1) + j];
    }
    part[wave][lane] = s;
    __syncthreads();
    if (wave != 0 || j > W) return;
    s = 0;
#pragma unroll
    for (int k = 0; k < WAVES; k++) s += part[k][lane];
    if (j == W) {
        meta[0] += (unsigned long long)origin;
        meta[1] += 1;
        meta[2] += s;
        return;
    }
    const int t = j / M, jj = j - t * M;
    const int g = jj / AMC_SAMPLE_Q, q = jj - g * AMC_SAMPLE_Q;
    const size_t at = ((size_t)g * (size_t)lags1 + (size_t)(t == 0 ? lag_a : lag_b)) * AMC_SAMPLE_Q + (size_t)q;
    amc_add128(tot[2 * at], tot[2 * at + 1], s);
}

hipError_t amc_launch_sample_reduce(amc_ctx *c, const unsigned long long *slab, int rows, int M, int tables, int lag_a, int lag_b,
                                    int lags1, int origin, unsigned long long *tot, unsigned long long *meta)
{
    amc_prof_begin(c, AMC_K_FIELDS);
    AMC_LAUNCH(c, k_sample_reduce, dim3((tables * M + 1 + 63) / 64), dim3(AMC_SAMPLE_REDUCE_THREADS), slab, rows, M, tables, lag_a, lag_b,
               lags1, origin, tot, meta);
    amc_prof_end(c);
    return hipGetLastError();
}

static int fields_enqueue(amc_ctx *c)
{
    amc_fields_ws &F = c->F;
    int blocks;
    if (int rc = amc_sample_blocks(c, "amc_fields", F.blocks_env, F.max_blocks, &blocks)) return rc;
    amc_prof_begin(c, AMC_K_FIELDS);
    AMC_LAUNCH(c, k_fields_accum, dim3(blocks), dim3(AMC_FIELDS_THREADS), c->S, amc_sample_lazy(c), (long long)c->lo, (long long)c->hi, F.G,
               F.slab, F.meta + 3);
    amc_prof_end(c);
    AMC_HIP(c, hipGetLastError());
    AMC_HIP(c, amc_launch_sample_reduce(c, F.slab, blocks, F.G.bins * AMC_FIELDS_Q, 1, 0, 0, 1, 0, F.tot, F.meta));
    return AMC_OK;
}

static void fields_free(amc_ctx *c)
{
    ctx_free(c, c->F.slab, c->F.tot, c->F.meta);
    c->F = amc_fields_ws();
}

// meta: [0] unused, [1] samples, [2] particles outside, [3] the error word (the layout k_sample_reduce writes)
static amc_totals fields_totals(const amc_fields_ws &F) { return amc_totals{F.tot, (size_t)2 * AMC_FIELDS_Q * (size_t)F.G.bins, F.meta, 4, 3}; }

extern "C" {

int amc_fields_step(amc_ctx *c)
{
    if (!amc_fields_due(c, c->out.step)) return AMC_OK;
    return fields_enqueue(c);
}

int amc_fields_config(amc_ctx *c, const amc_field_grid *g)
{
    if (!c) return AMC_ERR_INVALID;
    AMC_HIP(c, hipSetDevice(c->device));
    AMC_HIP(c, hipStreamSynchronize(c->stream));        // (a sample in flight may still use the old buffers)
    if (!g) {
        fields_free(c);
        return AMC_OK;
    }
    if (g->struct_size != (int32_t)sizeof(amc_field_grid)) return amc_fail(c, AMC_ERR_INVALID, "amc_field_grid.struct_size mismatch (ABI)");
    amc_fields_grid_dev G;
    if (int rc = amc_sample_grid_check(c, "amc_field_grid", "bins", g->kind, g->n1, g->n2, g->n3, AMC_FIELDS_MAX_BINS, g->lo, g->hi, g->every,
                                       g->step_offset, g->reserved == 0, nullptr, &G))
        return rc;
    fields_free(c);
    amc_fields_ws &F = c->F;
    F.g = *g;
    F.G = G;
    amc_sample_blocks_config(c, "AMC_FIELDS_BLOCKS", &F.blocks_env, &F.max_blocks);
    const size_t M = (size_t)G.bins * AMC_FIELDS_Q;
    if (dalloc(c, &F.slab, (size_t)F.max_blocks * (M + 1)) != hipSuccess || dalloc(c, &F.tot, 2 * M) != hipSuccess ||
        dalloc(c, &F.meta, 4) != hipSuccess) {
        fields_free(c);
        return amc_fail(c, AMC_ERR_HIP, "amc_fields_config: device allocation failed");
    }
    F.on = true;
    if (int rc = amc_fields_reset(c)) { fields_free(c); return rc; }
    return AMC_OK;
}

int amc_fields_sample(amc_ctx *c)
{
    if (!c) return AMC_ERR_INVALID;
    if (!c->F.on) return amc_fail(c, AMC_ERR_STATE, "amc_fields_sample before amc_fields_config");
    if (!c->uploaded) return amc_fail(c, AMC_ERR_STATE, "amc_fields_sample before amc_upload");
    AMC_HIP(c, hipSetDevice(c->device));
    return fields_enqueue(c);
}

int amc_fields_read(amc_ctx *c, int64_t *totals, int64_t *n_samples, int64_t *n_outside)
{
    if (!c) return AMC_ERR_INVALID;
    if (!c->F.on) return amc_fail(c, AMC_ERR_STATE, "amc_fields_read before amc_fields_config");
    AMC_HIP(c, hipSetDevice(c->device));
    unsigned long long meta[4], bad;
    if (int rc = amc_totals_get(c, fields_totals(c->F), totals, meta, &bad)) return rc;
    if (bad != ~0ULL)
        return amc_fail(c, AMC_ERR_CAPACITY, "amc_fields: particle %llu has a velocity component outside |c| < 2^14 m/s (or NaN); "
                        "sampling stopped until amc_fields_reset", bad);
    if (n_samples) *n_samples = (int64_t)meta[1];
    if (n_outside) *n_outside = (int64_t)meta[2];
    return AMC_OK;
}

int amc_fields_load(amc_ctx *c, const int64_t *totals, int64_t n_samples, int64_t n_outside)
{
    if (!c || !totals || n_samples < 0 || n_outside < 0) return AMC_ERR_INVALID;
    if (!c->F.on) return amc_fail(c, AMC_ERR_STATE, "amc_fields_load before amc_fields_config");
    AMC_HIP(c, hipSetDevice(c->device));
    const unsigned long long meta[4] = {0, (unsigned long long)n_samples, (unsigned long long)n_outside, 0};
    return amc_totals_put(c, fields_totals(c->F), totals, meta);
}

int amc_fields_reset(amc_ctx *c)
{
    if (!c) return AMC_ERR_INVALID;
    if (!c->F.on) return amc_fail(c, AMC_ERR_STATE, "amc_fields_reset before amc_fields_config");
    AMC_HIP(c, hipSetDevice(c->device));
    const unsigned long long meta[4] = {0, 0, 0, 0};
    return amc_totals_put(c, fields_totals(c->F), nullptr, meta);
}

}  // extern "C"
