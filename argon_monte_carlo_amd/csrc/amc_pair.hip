// amc_pair.hip — the sampled pair distribution: per region of a spatial grid, a histogram of the distance from every particle of
// the region (a centre, of the context's index range) to every other particle of the system, and of the pairs that still
// approach, accumulated as exact integer counts (include/argonmc_pair.h).  The reference has no such output; the
// Python layer derives g(r), the coordination number and the overlap diagnostics from the totals.
//
// The sampler owns its search structure (the step's kept per-cell lists have another cell edge and another life): cells with
// an edge above r_max over the grid's bounding box grown by r_max, rebuilt by every sample.  One sample is six kernels:
//   k_pair_file     one thread per particle of the SYSTEM: position through the deferred results, its cell (or none: unfiled),
//                   one returning atomic on the cell's count — the value is the particle's place in the cell; counts the
//                   particles of the range outside the grid and the unfiled ones.
//   k_pair_scan_sums, k_pair_scan   up to 128 workgroups: the sums of the waves' segments of cells, then the exclusive scan of the
//                   cell counts into cell_off, and the counts back to zero.
//   k_pair_scatter  one thread per particle: the record (index, region, x y z vx vy vz) to cell_off[cell] + place.  The records
//                   of a cell are contiguous, and so are those of cells adjacent along the last axis.
//   k_pair_count    a persistent grid of at most one workgroup per CU; every WAVE takes home cells in cell order, the next
//                   one from a shared cursor whenever it is done with its own (cells differ in cost by orders of magnitude:
//                   the gas fills a part of the box).  It holds a tile of up to 64 centres of the home cell in its lanes'
//                   registers, streams the records of the 3 x 3 runs of neighbouring cells (clipped at the box faces) through
//                   its lanes, 64 at a time, and tests the tile's centres one after the other against the lanes' neighbours:
//                   the centre is broadcast with v_readlane, the distance is tested in registers, a hit adds into the
//                   workgroup's table of 64-bit counters in LDS (LDS atomics whose result nobody reads: exact and order-free).
//                   One slab row per workgroup, plain stores.
//   k_slab_reduce<unsigned long long, pair_sink>  (amc_sample_dev.h) sums the slab rows per column; the sink adds the result into
//                   the 64-bit running totals, and one thread folds the two side counters in.  No global atomic touches the totals.
// Integer sums do not depend on the order of the adds, so the totals are bitwise the same for any number of workgroups, any
// order within a cell and any split of the index range.
#include <float.h>

#include "amc_host.h"
#include "amc_sample_dev.h"
#include "amc_cells_dev.h"

#define AMC_PAIR_THREADS 1024           // k_pair_count: the 48 KiB table leaves room for one workgroup per CU: 16 waves
#define AMC_PAIR_WAVES (AMC_PAIR_THREADS / 64)
#define AMC_PAIR_FILE_THREADS 256
// Why the table's counters are 64-bit: a centre adds one per neighbour within r_max, and nothing bounds how many particles a
// crafted state puts into one ball — 2^17 particles in one cell are 2^34 ordered pairs in one column of one workgroup.
static_assert(AMC_PAIR_MAX_COLUMNS * sizeof(unsigned long long) == 48 * 1024, "the table is 48 KiB of LDS");
static_assert(1 + 2 * AMC_PAIR_MAX_HIST_BINS <= AMC_PAIR_MAX_COLUMNS, "one region of the longest histogram fits the table");
static_assert((long long)AMC_PAIR_MAX_CELLS_AXIS * AMC_PAIR_MAX_CELLS_AXIS * AMC_PAIR_MAX_CELLS_AXIS <= (1LL << 21), "cell indices fit an int with room to spare");

// the grid as the kernels take it
struct amc_pair_dev {
    amc_fields_grid_dev G;              // the regions
    amc_fields_grid_dev B;              // the search box: a Cartesian grid of cells, linear index (cx * n2 + cy) * n3 + cz
    int H, C;                           // columns of the histogram, columns per region: 1 + 2 * H
    double r_max, wr;                   // wr = r_max / H
    double r2_skip;                     // r2 above this: sqrt(r2) >= r_max for sure (the exact rule decides the rest)
};

AMC_DEV void pair_add(unsigned long long *p) { (void)__hip_atomic_fetch_add(p, 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__global__ __launch_bounds__(AMC_PAIR_FILE_THREADS) void k_pair_file(amc_state S, amc_lazy L, long long n, long long lo, long long hi,
                                                                     amc_pair_dev V, unsigned int *cell_count, int *cell_of, int *rank_of,
                                                                     unsigned long long *side)
{
    __shared__ unsigned int outside_sum, unfiled_sum;
    if (threadIdx.x == 0) { outside_sum = 0; unfiled_sum = 0; }
    __syncthreads();
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n) {
        double x = amc_g(S.x)[p], y = amc_g(S.y)[p], z = amc_g(S.z)[p], vx = 0.0, vy = 0.0, vz = 0.0;
        amc_fields_lazy(L, p, x, y, z, vx, vy, vz);
        const int cell = amc_sample_bin(V.B, x, y, z);
        int rank = 0;
        if (cell >= 0) {
            rank = (int)__hip_atomic_fetch_add(amc_g(cell_count) + cell, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (p >= lo && p < hi && amc_sample_bin(V.G, x, y, z) < 0) atomicAdd(&outside_sum, 1u);
        } else {
            atomicAdd(&unfiled_sum, 1u);
        }
        amc_g(cell_of)[p] = cell;
        amc_g(rank_of)[p] = rank;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (outside_sum) (void)__hip_atomic_fetch_add(amc_g(side), (unsigned long long)outside_sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (unfiled_sum) (void)__hip_atomic_fetch_add(amc_g(side) + 1, (unsigned long long)unfiled_sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// (the exclusive scan of the cells' counts, k_pair_scan_sums and k_pair_scan with pair_scan_geometry: amc_cells_dev.h)

__global__ __launch_bounds__(AMC_PAIR_FILE_THREADS) void k_pair_scatter(amc_state S, amc_lazy L, long long n, amc_pair_dev V,
                                                                        const unsigned int *cell_off, const int *cell_of, const int *rank_of,
                                                                        int2 *rec_ir, double *rec_s)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int cell = amc_g(cell_of)[p];
    if (cell < 0) return;
    const size_t dst = (size_t)amc_g(cell_off)[cell] + (size_t)amc_g(rank_of)[p];     // (below the number of filed particles <= n)
    double x = amc_g(S.x)[p], y = amc_g(S.y)[p], z = amc_g(S.z)[p], vx = amc_g(S.vx)[p], vy = amc_g(S.vy)[p], vz = amc_g(S.vz)[p];
    amc_fields_lazy(L, p, x, y, z, vx, vy, vz);
    int2 ir;
    ir.x = (int)p;
    ir.y = amc_sample_bin(V.G, x, y, z);
    amc_g_store(rec_ir + dst, ir);
    auto *r = amc_g(rec_s) + dst;
    r[0] = x; r[(size_t)n] = y; r[2 * (size_t)n] = z; r[3 * (size_t)n] = vx; r[4 * (size_t)n] = vy; r[5 * (size_t)n] = vz;
}

// One home cell h (records [h0, h1)) by one wave; everything but `lane` and what is loaded per lane is wave-uniform.
AMC_DEV void pair_home(const amc_pair_dev &V, unsigned long long *tab, int lane, int h, unsigned int h0, unsigned int h1, long long n, int lo,
                       int hi, const unsigned int *cell_off, const int2 *rec_ir, const double *rec_s)
{
    const int n1 = V.B.n1, n2 = V.B.n2, n3 = V.B.n3, H = V.H, C = V.C;
    const int cz = h % n3, cy = (h / n3) % n2, cx = h / (n3 * n2);
    const auto *off = amc_g(cell_off);
    const auto *gs = amc_g(rec_s);
    const size_t N = (size_t)n;
    for (unsigned int ct = h0; ct < h1; ct += 64) {
        // the tile's centres, one per lane
        const unsigned int ci = ct + (unsigned int)lane;
        int c_idx = -1, c_reg = -1;
        double c_x = 0.0, c_y = 0.0, c_z = 0.0, c_vx = 0.0, c_vy = 0.0, c_vz = 0.0;
        if (ci < h1) {
            const int2 ir = amc_g_load(rec_ir + ci);
            if (ir.x >= lo && ir.x < hi && ir.y >= 0) {
                c_idx = ir.x; c_reg = ir.y;
                c_x = gs[ci]; c_y = gs[N + ci]; c_z = gs[2 * N + ci]; c_vx = gs[3 * N + ci]; c_vy = gs[4 * N + ci]; c_vz = gs[5 * N + ci];
                pair_add(tab + c_reg * C);
            }
        }
        const unsigned long long centres = __ballot(c_reg >= 0);
        if (!centres) continue;
        // the 3 x 3 runs of cells around the home cell, clipped at the box faces: cells adjacent along z are one run of records
        const int zl = max(cz - 1, 0), zh = min(cz + 1, n3 - 1);
        for (int X = max(cx - 1, 0); X <= min(cx + 1, n1 - 1); X++)
            for (int Y = max(cy - 1, 0); Y <= min(cy + 1, n2 - 1); Y++) {
                const int row = (X * n2 + Y) * n3;
                const unsigned int j0 = off[row + zl], j1 = off[row + zh + 1];
                for (unsigned int jb = j0; jb < j1; jb += 64) {
                    const unsigned int j = jb + (unsigned int)lane;
                    const bool have = j < j1;
                    int n_idx = -1;
                    double n_x = 0.0, n_y = 0.0, n_z = 0.0, n_vx = 0.0, n_vy = 0.0, n_vz = 0.0;
                    if (have) {
                        n_idx = amc_g_load(rec_ir + j).x;
                        n_x = gs[j]; n_y = gs[N + j]; n_z = gs[2 * N + j]; n_vx = gs[3 * N + j]; n_vy = gs[4 * N + j]; n_vz = gs[5 * N + j];
                    }
                    for (unsigned long long m = centres; m; m &= m - 1) {
                        const int k = __builtin_amdgcn_readfirstlane(__ffsll((long long)m) - 1);
                        const int i_idx = __builtin_amdgcn_readlane(c_idx, k), i_reg = __builtin_amdgcn_readlane(c_reg, k);
                        const double dx = pair_lane(c_x, k) - n_x, dy = pair_lane(c_y, k) - n_y, dz = pair_lane(c_z, k) - n_z;
                        const double r2 = (dx * dx + dy * dy) + dz * dz;
                        if (!have || n_idx == i_idx || r2 > V.r2_skip) continue;
                        const double r = sqrt(r2);
                        if (!(r < V.r_max)) continue;
                        const int col = amc_fields_axis(r, 0.0, V.r_max, V.wr, H);
                        if (col < 0) continue;      // (cannot happen: r < r_max puts floor(r / wr) at H at the most)
                        const double dvx = pair_lane(c_vx, k) - n_vx, dvy = pair_lane(c_vy, k) - n_vy, dvz = pair_lane(c_vz, k) - n_vz;
                        const double s = (dx * dvx + dy * dvy) + dz * dvz;
                        unsigned long long *a = tab + i_reg * C + 1 + col;
                        pair_add(a);
                        if (s < 0.0) pair_add(a + H);
                    }
                }
            }
    }
}

// chunk: consecutive cells a wave takes at a time (1 .. 64: lane b < chunk reads cell b's bounds; pair_enqueue chooses it).
// cursor: the next chunk nobody has taken yet, zero at the launch (pair_sink puts it back); who takes which chunk changes
// from launch to launch, the sums do not.
__global__ __launch_bounds__(AMC_PAIR_THREADS) void k_pair_count(amc_pair_dev V, long long n, int lo, int hi, int chunk, const unsigned int *cell_off,
                                                                 const int2 *rec_ir, const double *rec_s, unsigned long long *slab,
                                                                 unsigned long long *cursor)
{
    __shared__ unsigned long long tab[AMC_PAIR_MAX_COLUMNS];    // G.bins * C counters (the sampler's column limit)
    const int M = V.G.bins * V.C;
    amc_slab_begin(tab, M);
    const int lane = threadIdx.x & 63;
    const int ncells = V.B.bins;
    for (;;) {
        unsigned long long take = 0;
        if (lane == 0) take = __hip_atomic_fetch_add(amc_g(cursor), 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const long long base = (long long)__builtin_amdgcn_readfirstlane((int)take) * chunk;     // (at most cells + waves chunks are ever taken)
        if (base >= ncells) break;
        const int cell = (int)base + lane;
        unsigned int c0 = 0, c1 = 0;
        if (lane < chunk && cell < ncells) { c0 = amc_g(cell_off)[cell]; c1 = amc_g(cell_off)[cell + 1]; }
        for (unsigned long long live = __ballot(c1 > c0); live; live &= live - 1) {
            const int b = __builtin_amdgcn_readfirstlane(__ffsll((long long)live) - 1);
            pair_home(V, tab, lane, (int)base + b, __builtin_amdgcn_readlane(c0, b), __builtin_amdgcn_readlane(c1, b), n, lo, hi, cell_off, rec_ir,
                      rec_s);
        }
    }
    amc_slab_store(slab, tab, M);
}

// the pair distribution's end of k_slab_reduce: column j is the totals' (region, column) j; the counters' thread counts the sample
// and folds the side counters in (and zeroes them, and k_pair_count's cursor, for the next sample).  It never stops.
// meta: [0] unused, [1] samples, [2] particles outside, [3] particles unfiled
struct pair_sink {
    static constexpr bool companion = false;
    unsigned long long *tot, *meta, *side;
    AMC_DEV bool stopped() const { return false; }
    AMC_DEV int stride(int W) const { return W; }
    AMC_DEV void column(int j, unsigned long long s) const { amc_g(tot)[j] += s; }
    AMC_DEV void counters(unsigned long long) const
    {
        amc_g(meta)[1] += 1;
        amc_g(meta)[2] += amc_g(side)[0];
        amc_g(meta)[3] += amc_g(side)[1];
        amc_g(side)[0] = 0;
        amc_g(side)[1] = 0;
        amc_g(side)[2] = 0;             // k_pair_count's cursor
    }
};

// ---- the host side -------------------------------------------------------------------------------------------------------------
// A shard of a pore geometry cannot sample: its step ends with the owner's bounds pass over [lo, hi) (amc_mg_finish), which
// consumes the sweep's deferred results and recaptures the owner's particles only — the final state of the OTHER shards'
// particles, which every centre needs for its neighbours, reaches this rank with the next exchange.  (The cube has no such pass:
// the deferred results of the whole system are still pending at the hook.  One rank over the whole range owns everybody.)
static int pair_shard_ok(amc_ctx *c, const char *who)
{
    if (c->P.geometry == AMC_GEOM_CUBE || (c->lo == 0 && c->hi == c->n)) return AMC_OK;
    return amc_fail(c, AMC_ERR_STATE, "%s: the pair distribution cannot be sampled on an index-range shard [%lld, %lld) of a pore geometry "
                    "(the other shards' final state of a step is not resident); sample on one context, or in the cube", who, (long long)c->lo,
                    (long long)c->hi);
}

// the scratch words every sample expects at zero (the scan and the reduce of a completed sample leave them so)
static int pair_clear_scratch(amc_ctx *c)
{
    amc_pair_ws &F = c->PD;
    AMC_HIP(c, hipMemsetAsync(F.cell_count, 0, sizeof(unsigned int) * (size_t)F.B.bins, c->stream));
    AMC_HIP(c, hipMemsetAsync(F.side, 0, 3 * sizeof(unsigned long long), c->stream));
    return AMC_OK;
}

static int pair_launches(amc_ctx *c);

int amc_pair_enqueue(amc_ctx *c)       // (AMC_INTERNAL: the cadence hook's)
{
    amc_pair_ws &F = c->PD;
    if (int rc = pair_shard_ok(c, "amc_pair")) return rc;
    if (c->n > AMC_SAMPLE_MAX_PARTICLES)
        return amc_fail(c, AMC_ERR_CAPACITY, "amc_pair: %lld particles in the system (at most 2^24)", (long long)c->n);
    // a sample whose launches failed half-way left counts, side words or the cursor behind: the next one starts from zero again
    if (F.dirty) { if (int rc = pair_clear_scratch(c)) return rc; }
    F.dirty = true;
    if (int rc = pair_launches(c)) return rc;
    F.dirty = false;
    return AMC_OK;
}

static int pair_launches(amc_ctx *c)
{
    amc_pair_ws &F = c->PD;
    amc_pair_dev V;
    V.G = F.G; V.B = F.B; V.H = F.g.hist_bins; V.C = F.C; V.r_max = F.g.r_max; V.wr = F.wr;
    const double rm2 = F.g.r_max * F.g.r_max;
    V.r2_skip = (isfinite(rm2) && rm2 >= DBL_MIN * 0x1p64) ? rm2 * 1.000001 : INFINITY;
    const int W = F.G.bins * F.C, ncells = F.B.bins;
    const int blocks = F.blocks_env > 0 ? std::min(F.blocks_env, F.max_blocks) : F.max_blocks;
    // cells a wave takes at a time: one, unless that made more than 16 takes per wave — every take is an atomic on ONE word, and
    // a grid at the cap of 128 cells per axis, mostly empty, would spend its time there
    const int chunk = (int)std::max<long long>(1, std::min<long long>(64, ncells / ((long long)blocks * AMC_PAIR_WAVES * 16)));
    // (an empty system still launches one workgroup, which finds no particle: a grid of zero workgroups is an invalid launch)
    const unsigned int pblocks = (unsigned int)std::max<long long>(1, (c->n + AMC_PAIR_FILE_THREADS - 1) / AMC_PAIR_FILE_THREADS);
    const amc_lazy L = amc_sample_lazy(c);
    int sblocks, seg;
    pair_scan_geometry(ncells, &sblocks, &seg);
    amc_prof_begin(c, AMC_K_FIELDS);
    AMC_LAUNCH(c, k_pair_file, dim3(pblocks), dim3(AMC_PAIR_FILE_THREADS), c->S, L, (long long)c->n, (long long)c->lo, (long long)c->hi, V,
               F.cell_count, F.cell_of, F.rank_of, F.side);
    amc_prof_end(c);
    AMC_HIP(c, hipGetLastError());
    amc_prof_begin(c, AMC_K_FIELDS);
    AMC_LAUNCH(c, k_pair_scan_sums, dim3(sblocks), dim3(AMC_PAIR_SCAN_THREADS), (const unsigned int *)F.cell_count, F.wave_sum, ncells, seg);
    amc_prof_end(c);
    AMC_HIP(c, hipGetLastError());
    amc_prof_begin(c, AMC_K_FIELDS);
    AMC_LAUNCH(c, k_pair_scan, dim3(sblocks), dim3(AMC_PAIR_SCAN_THREADS), F.cell_count, F.cell_off, (const unsigned int *)F.wave_sum, ncells, seg);
    amc_prof_end(c);
    AMC_HIP(c, hipGetLastError());
    amc_prof_begin(c, AMC_K_FIELDS);
    AMC_LAUNCH(c, k_pair_scatter, dim3(pblocks), dim3(AMC_PAIR_FILE_THREADS), c->S, L, (long long)c->n, V, (const unsigned int *)F.cell_off,
               (const int *)F.cell_of, (const int *)F.rank_of, F.rec_ir, F.rec_s);
    amc_prof_end(c);
    AMC_HIP(c, hipGetLastError());
    amc_prof_begin(c, AMC_K_FIELDS);
    AMC_LAUNCH(c, k_pair_count, dim3(blocks), dim3(AMC_PAIR_THREADS), V, (long long)c->n, (int)c->lo, (int)c->hi, chunk,
               (const unsigned int *)F.cell_off, (const int2 *)F.rec_ir, (const double *)F.rec_s, F.slab, F.side + 2);
    amc_prof_end(c);
    AMC_HIP(c, hipGetLastError());
    AMC_HIP(c, amc_launch_slab_reduce(c, (const unsigned long long *)F.slab, blocks, W, pair_sink{F.tot, F.meta, F.side}));
    return AMC_OK;
}

static void pair_free(amc_ctx *c)
{
    amc_pair_ws &F = c->PD;
    ctx_free(c, F.cell_count, F.cell_off, F.wave_sum, F.cell_of, F.rank_of, F.rec_ir, F.rec_s, F.side, F.slab, F.tot, F.meta);
    c->PD = amc_pair_ws();
}

static amc_totals pair_totals(const amc_pair_ws &F) { return amc_totals{F.tot, (size_t)F.G.bins * (size_t)F.C, F.meta, 4, 0}; }

// The search box of grid G for r_max: the bounding box grown by r_max, min(floor(extent / (r_max * (1 + 2^-20))), 128) cells per
// axis (at least 1).  false: the box is not finite or a cell edge is not positive.
static bool pair_box(const amc_fields_grid_dev &G, double r_max, amc_fields_grid_dev *B)
{
    double lo[3], hi[3];
    if (G.kind == AMC_FIELDS_CARTESIAN) {
        for (int k = 0; k < 3; k++) { lo[k] = G.lo[k] - r_max; hi[k] = G.hi[k] + r_max; }
    } else {
        lo[0] = lo[1] = -G.hi[0] - r_max; hi[0] = hi[1] = G.hi[0] + r_max;
        lo[2] = G.lo[1] - r_max; hi[2] = G.hi[1] + r_max;
    }
    int n[3];
    const double edge = r_max * (1.0 + 0x1p-20);
    for (int k = 0; k < 3; k++) {
        const double ext = hi[k] - lo[k];
        if (!(isfinite(ext) && ext > 0.0 && edge > 0.0)) return false;
        const double f = floor(ext / edge);
        n[k] = f >= (double)AMC_PAIR_MAX_CELLS_AXIS ? AMC_PAIR_MAX_CELLS_AXIS : f >= 1.0 ? (int)f : 1;
        B->lo[k] = lo[k]; B->hi[k] = hi[k]; B->w[k] = ext / (double)n[k];
        if (!(B->w[k] > 0.0 && isfinite(B->w[k]))) return false;
    }
    B->kind = AMC_FIELDS_CARTESIAN; B->n1 = n[0]; B->n2 = n[1]; B->n3 = n[2]; B->bins = n[0] * n[1] * n[2];
    return true;
}

extern "C" {

int amc_pair_reset(amc_ctx *c)
{
    if (!c) return AMC_ERR_INVALID;
    if (int rc = amc_sampler_ready(c, c->PD.on, "amc_pair", "reset")) return rc;
    const unsigned long long meta[4] = {0, 0, 0, 0};
    return amc_totals_put(c, pair_totals(c->PD), nullptr, meta);
}

int amc_pair_config(amc_ctx *c, const amc_pair_grid *g)
{
    bool done;
    if (int rc = amc_sampler_config_begin(c, g, "amc_pair_grid", pair_free, &done); rc || done) return rc;
    const char *fault = nullptr;
    if (g->hist_bins < 1 || g->hist_bins > AMC_PAIR_MAX_HIST_BINS) fault = "hist_bins must be 1 .. 256";
    else if (!(isfinite(g->r_max) && g->r_max > 0.0)) fault = "r_max must be finite and > 0";
    const int C = 1 + 2 * (g->hist_bins >= 1 && g->hist_bins <= AMC_PAIR_MAX_HIST_BINS ? g->hist_bins : 1);
    amc_fields_grid_dev G, B;
    if (int rc = amc_sample_grid_check(c, "amc_pair_grid", "regions (1 + 2 * hist_bins columns each, 6,144 columns in all)", g->kind, g->n1, g->n2,
                                       g->n3, AMC_PAIR_MAX_COLUMNS / C, g->lo, g->hi, g->every, g->step_offset,
                                       g->reserved[0] == 0 && g->reserved[1] == 0, fault, &G))
        return rc;
    if (!pair_box(G, g->r_max, &B) || !(g->r_max / (double)g->hist_bins > 0.0))
        return amc_fail(c, AMC_ERR_INVALID, "amc_pair_grid: r_max %g gives no finite search box with positive cell edges and columns", g->r_max);
    if (c->n > AMC_SAMPLE_MAX_PARTICLES)
        return amc_fail(c, AMC_ERR_CAPACITY, "amc_pair: %lld particles in the system (at most 2^24)", (long long)c->n);
    if (int rc = pair_shard_ok(c, "amc_pair_config")) return rc;
    pair_free(c);
    amc_pair_ws &F = c->PD;
    F.g = *g;
    F.G = G;
    F.B = B;
    F.C = C;
    F.wr = g->r_max / (double)g->hist_bins;
    amc_sample_blocks_config(c, "AMC_PAIR_BLOCKS", &F.blocks_env, &F.max_blocks);
    const size_t n = (size_t)std::max<int64_t>(c->n, 1), cells = (size_t)B.bins;
    if (dalloc(c, &F.cell_count, cells) != hipSuccess || dalloc(c, &F.cell_off, cells + 1) != hipSuccess ||
        dalloc(c, &F.wave_sum, (size_t)AMC_PAIR_SCAN_MAX_BLOCKS * AMC_PAIR_SCAN_WAVES) != hipSuccess || dalloc(c, &F.cell_of, n) != hipSuccess ||
        dalloc(c, &F.rank_of, n) != hipSuccess || dalloc(c, &F.rec_ir, n) != hipSuccess || dalloc(c, &F.rec_s, 6 * n) != hipSuccess ||
        dalloc(c, &F.side, 3) != hipSuccess || dalloc(c, &F.slab, (size_t)F.max_blocks * (size_t)G.bins * C) != hipSuccess ||
        dalloc(c, &F.tot, pair_totals(F).words) != hipSuccess || dalloc(c, &F.meta, 4) != hipSuccess) {
        pair_free(c);
        return amc_fail(c, AMC_ERR_HIP, "amc_pair_config: device allocation failed");
    }
    if (int rc = pair_clear_scratch(c)) { pair_free(c); return rc; }
    F.on = true;
    if (int rc = amc_pair_reset(c)) { pair_free(c); return rc; }
    return AMC_OK;
}

int amc_pair_sample(amc_ctx *c)
{
    if (!c) return AMC_ERR_INVALID;
    if (int rc = amc_sampler_sample_ready(c, c->PD.on, "amc_pair")) return rc;
    return amc_pair_enqueue(c);
}

int amc_pair_read(amc_ctx *c, int64_t *totals, int64_t *n_samples, int64_t *n_outside, int64_t *n_unfiled)
{
    if (!c) return AMC_ERR_INVALID;
    if (int rc = amc_sampler_ready(c, c->PD.on, "amc_pair", "read")) return rc;
    unsigned long long meta[4], bad;
    if (int rc = amc_totals_get(c, pair_totals(c->PD), totals, meta, &bad)) return rc;
    if (n_samples) *n_samples = (int64_t)meta[1];
    if (n_outside) *n_outside = (int64_t)meta[2];
    if (n_unfiled) *n_unfiled = (int64_t)meta[3];
    return AMC_OK;
}

int amc_pair_load(amc_ctx *c, const int64_t *totals, int64_t n_samples, int64_t n_outside, int64_t n_unfiled)
{
    if (!c || !totals || n_samples < 0 || n_outside < 0 || n_unfiled < 0) return AMC_ERR_INVALID;
    if (int rc = amc_sampler_ready(c, c->PD.on, "amc_pair", "load")) return rc;
    const unsigned long long meta[4] = {0, (unsigned long long)n_samples, (unsigned long long)n_outside, (unsigned long long)n_unfiled};
    return amc_totals_put(c, pair_totals(c->PD), totals, meta);
}

}  // extern "C"
