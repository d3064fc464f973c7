// amc_fields.hip — sampled fields: per spatial bin, the particle count and the first and second moments of the velocity
// components, accumulated as exact integers (include/argonmc.h "sampled fields").  The reference has no such
// output; the Python layer derives number density, flow velocity and temperature from the totals.
//
// One sample is two kernels:
//   k_fields_accum   a persistent grid of at most one workgroup per CU.  Each workgroup streams a contiguous index range
//                    (x, y, z, vx, vy, vz: 48 B per particle, 16-B loads of particle pairs), computes the bin and the seven
//                    integers of each particle and adds them into a table in LDS (64-bit integer LDS atomics: exact and
//                    order-free).  It stores the table as one slab row with plain stores — no global atomics.
//   k_fields_reduce  sums the slab rows per (bin, quantity) and adds the result into the 128-bit running totals.
// Integer sums do not depend on the order of the adds, so the totals are bitwise the same for any number of workgroups.
#include "amc_host.h"
#include "amc_sample_dev.h"

#define AMC_FIELDS_Q 7                  // count, q1(c1..c3), q2(c1..c3)
#define AMC_FIELDS_THREADS 1024         // the 112 KiB table leaves room for one workgroup per CU: 16 waves
#define AMC_FIELDS_PER_BLOCK 8192       // particles per workgroup below which fewer workgroups are launched
#define AMC_FIELDS_MAX_PARTICLES (1LL << 24)

// one particle into the workgroup's table; returns false if a component is out of the quantisation range
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
    if (!(fabs(c1) < 16384.0) || !(fabs(c2) < 16384.0) || !(fabs(c3) < 16384.0)) return false;
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

// column j of the slab (j < M: (bin, quantity) j, j == M: particles outside) summed over the rows -> running totals.
// 64 columns per workgroup, its four waves take every fourth row.
__global__ __launch_bounds__(256) void k_fields_reduce(const unsigned long long *slab, int rows, int M, unsigned long long *tot,
                                                       unsigned long long *meta)
{
    if (meta[2] != ~0ULL) return;       // a sample with a particle out of range adds nothing (amc_fields_read reports it)
    __shared__ unsigned long long part[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + lane;
    unsigned long long s = 0;           // (wraps modulo 2^64; the true sum of one sample is below 2^62 in magnitude)
    if (j <= M)
        for (int b = wave; b < rows; b += 4) s += slab[(size_t)b * (size_t)(M + 1) + j];
    part[wave][lane] = s;
    __syncthreads();
    if (wave != 0 || j > M) return;
    s = part[0][lane] + part[1][lane] + part[2][lane] + part[3][lane];
    if (j == M) {
        meta[0] += 1;
        meta[1] += s;
        return;
    }
    const unsigned long long old = tot[2 * j], now = old + s;
    tot[2 * j] = now;
    tot[2 * j + 1] += (unsigned long long)(((long long)s < 0 ? -1LL : 0LL) + (now < old ? 1LL : 0LL));
}

static int fields_enqueue(amc_ctx *c)
{
    amc_fields_ws &F = c->F;
    const long long cnt = c->hi - c->lo;
    if (cnt > AMC_FIELDS_MAX_PARTICLES)
        return amc_fail(c, AMC_ERR_CAPACITY, "amc_fields: %lld particles in one sample (at most 2^24 keep the sums exact)", cnt);
    int blocks = F.blocks_env > 0 ? F.blocks_env : (int)std::min<long long>(F.max_blocks, std::max<long long>(1, (cnt + AMC_FIELDS_PER_BLOCK - 1) / AMC_FIELDS_PER_BLOCK));
    blocks = std::min(blocks, F.max_blocks);
    amc_lazy L;
    memset(&L, 0, sizeof L);
    if (c->step.lazy_pending) { L.slot_of = c->W.slot_of; L.state = c->W.sl_state; L.moved = c->W.sl_moved; L.enabled = 1; }
    amc_fields_grid_dev G;
    G.kind = F.g.kind; G.n1 = F.g.n1; G.n2 = F.g.n2; G.n3 = F.g.n3; G.bins = F.bins;
    for (int k = 0; k < 3; k++) { G.lo[k] = F.g.lo[k]; G.hi[k] = F.g.hi[k]; G.w[k] = F.w[k]; }
    const int M = F.bins * AMC_FIELDS_Q;
    amc_prof_begin(c, AMC_K_FIELDS);
    AMC_LAUNCH(c, k_fields_accum, dim3(blocks), dim3(AMC_FIELDS_THREADS), c->S, L, (long long)c->lo, (long long)c->hi, G, F.slab,
               F.meta + 2);
    amc_prof_end(c);
    AMC_HIP(c, hipGetLastError());
    amc_prof_begin(c, AMC_K_FIELDS);
    AMC_LAUNCH(c, k_fields_reduce, dim3((M + 1 + 63) / 64), dim3(256), (const unsigned long long *)F.slab, blocks, M, F.tot, F.meta);
    amc_prof_end(c);
    AMC_HIP(c, hipGetLastError());
    return AMC_OK;
}

static void fields_free(amc_ctx *c)
{
    ctx_free(c, c->F.slab, c->F.tot, c->F.meta);
    c->F = amc_fields_ws();
}

static int fields_clear(amc_ctx *c)
{
    amc_fields_ws &F = c->F;
    const unsigned long long meta[3] = {0, 0, ~0ULL};
    AMC_HIP(c, hipMemsetAsync(F.tot, 0, sizeof(unsigned long long) * 2 * AMC_FIELDS_Q * (size_t)F.bins, c->stream));
    AMC_HIP(c, hipMemcpyAsync(F.meta, meta, sizeof meta, hipMemcpyHostToDevice, c->stream));
    AMC_HIP(c, hipStreamSynchronize(c->stream));
    return AMC_OK;
}

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
    if (g->kind != AMC_FIELDS_CARTESIAN && g->kind != AMC_FIELDS_AXISYMMETRIC)
        return amc_fail(c, AMC_ERR_INVALID, "amc_field_grid.kind %d is neither Cartesian (0) nor axisymmetric (1)", g->kind);
    if (g->n1 < 1 || g->n2 < 1 || g->n3 < 1 || (long long)g->n1 * g->n2 * g->n3 > AMC_FIELDS_MAX_BINS)
        return amc_fail(c, AMC_ERR_INVALID, "amc_field_grid: %d x %d x %d bins (each >= 1, at most %d in all)", g->n1, g->n2, g->n3,
                        AMC_FIELDS_MAX_BINS);
    if (g->kind == AMC_FIELDS_AXISYMMETRIC && (g->n3 != 1 || g->lo[0] != 0.0))
        return amc_fail(c, AMC_ERR_INVALID, "amc_field_grid: an axisymmetric grid has n3 == 1 and r from lo[0] == 0");
    if (g->every < 0 || g->step_offset < 0 || g->reserved != 0)
        return amc_fail(c, AMC_ERR_INVALID, "amc_field_grid: every and step_offset must be >= 0, reserved 0");
    const int axes = g->kind == AMC_FIELDS_CARTESIAN ? 3 : 2;
    for (int k = 0; k < axes; k++)
        if (!(isfinite(g->lo[k]) && isfinite(g->hi[k]) && g->lo[k] < g->hi[k]))
            return amc_fail(c, AMC_ERR_INVALID, "amc_field_grid: axis %d needs finite bounds lo < hi", k + 1);
    fields_free(c);
    amc_fields_ws &F = c->F;
    F.g = *g;
    F.bins = g->n1 * g->n2 * g->n3;
    const int n[3] = {g->n1, g->n2, g->n3};
    for (int k = 0; k < 3; k++) F.w[k] = k < axes ? (g->hi[k] - g->lo[k]) / (double)n[k] : 1.0;
    if (g->kind == AMC_FIELDS_AXISYMMETRIC) { F.g.lo[2] = 0.0; F.g.hi[2] = 1.0; }
    F.blocks_env = getenv("AMC_FIELDS_BLOCKS") ? atoi(getenv("AMC_FIELDS_BLOCKS")) : 0;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess || cus < 1) cus = 256;
    F.max_blocks = F.blocks_env > 0 ? F.blocks_env : cus;
    const size_t M = (size_t)F.bins * AMC_FIELDS_Q;
    int rc = AMC_OK;
    if (dalloc(c, &F.slab, (size_t)F.max_blocks * (M + 1)) != hipSuccess || dalloc(c, &F.tot, 2 * M) != hipSuccess ||
        dalloc(c, &F.meta, 3) != hipSuccess) {
        fields_free(c);
        return amc_fail(c, AMC_ERR_HIP, "amc_fields_config: device allocation failed");
    }
    F.on = true;
    if ((rc = fields_clear(c))) { fields_free(c); return rc; }
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
    amc_fields_ws &F = c->F;
    unsigned long long meta[3];
    {
        amc_stage st(c);
        if (totals) AMC_HIP(c, st.get(totals, F.tot, sizeof(unsigned long long) * 2 * AMC_FIELDS_Q * (size_t)F.bins));
        AMC_HIP(c, st.get(meta, F.meta, sizeof meta));
        AMC_HIP(c, st.finish());
    }
    if (meta[2] != ~0ULL)
        return amc_fail(c, AMC_ERR_CAPACITY, "amc_fields: particle %llu has a velocity component outside |c| < 2^14 m/s (or NaN); "
                        "sampling stopped until amc_fields_reset", meta[2]);
    if (n_samples) *n_samples = (int64_t)meta[0];
    if (n_outside) *n_outside = (int64_t)meta[1];
    return AMC_OK;
}

int amc_fields_load(amc_ctx *c, const int64_t *totals, int64_t n_samples, int64_t n_outside)
{
    if (!c || !totals || n_samples < 0 || n_outside < 0) return AMC_ERR_INVALID;
    if (!c->F.on) return amc_fail(c, AMC_ERR_STATE, "amc_fields_load before amc_fields_config");
    AMC_HIP(c, hipSetDevice(c->device));
    amc_fields_ws &F = c->F;
    const unsigned long long meta[3] = {(unsigned long long)n_samples, (unsigned long long)n_outside, ~0ULL};
    AMC_HIP(c, hipMemcpyAsync(F.tot, totals, sizeof(unsigned long long) * 2 * AMC_FIELDS_Q * (size_t)F.bins, hipMemcpyHostToDevice,
                              c->stream));
    AMC_HIP(c, hipMemcpyAsync(F.meta, meta, sizeof meta, hipMemcpyHostToDevice, c->stream));
    AMC_HIP(c, hipStreamSynchronize(c->stream));
    return AMC_OK;
}

int amc_fields_reset(amc_ctx *c)
{
    if (!c) return AMC_ERR_INVALID;
    if (!c->F.on) return amc_fail(c, AMC_ERR_STATE, "amc_fields_reset before amc_fields_config");
    AMC_HIP(c, hipSetDevice(c->device));
    return fields_clear(c);
}

}  // extern "C"
