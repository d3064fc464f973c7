// amc_ic.hip — synthetic initial conditions generated on the device (include/argonmc.h, amc_ic_config).
// The recipe of the reference's generators (Cube:144-172, Pore:106-158) as restated in argon_monte_carlo_amd/ic.py —
// positions uniform per region (cube, or stacked cylinders with r = R sqrt(u), theta ~ U(0, 2 pi), z ~ U(z_lo, z_hi),
// Pore:120-139), velocity components N(0, a_shape^2) (= Maxwell speeds, isotropic; Pore:144-158), accumulators zero, flag
// clear — on a counter-based generator of its own: a particle's numbers depend on (seed, particle index) only, so every
// rank of a sharded run produces the identical system without moving 137 B per particle through PCIe.  NOT the
// reference's scipy / NumPy streams: opt-in, never what a parity test starts from.
//
// And the overlap removal of such a start (include/argonmc-ic.h): amc_init_separate searches the whole system for
// pairs closer than min_dist and redraws the atom of the higher index from the same recipe with the round number in the counter,
// round after round.  One search is six kernels over a work space that lives for the call:
//   k_ic_file       one thread per atom: its cell (clamped into the box), one returning atomic on the cell's count — the value is
//                   the atom's place in the cell; clears the atom's loser mark.
//   k_pair_scan_sums, k_pair_scan   (amc_cells_dev.h) the exclusive scan of the cell counts into cell_off.
//   k_ic_scatter    one thread per atom: the record (index; x, y, z) to cell_off[cell] + place.
//   k_ic_mark       a persistent grid; every WAVE takes home cells from a shared cursor, holds up to 64 centres of the home cell
//                   in its lanes, streams the records of the 3 x 3 runs of neighbouring cells (clipped at the box faces; cells
//                   adjacent along the last axis are one run) through its lanes and tests the centres one after the other
//                   against the lanes' neighbours: the centre is broadcast with v_readlane, the test is made in registers.  A
//                   hit with centre index < neighbour index stores 1 into lose[neighbour] — a plain store of a constant: order-
//                   free — and counts one pair: every unordered pair exactly once, from the home cell of its lower index.  The
//                   count is summed per workgroup and added once.
//   k_ic_redraw     one thread per atom: a loser is counted and, unless the budget of rounds is spent, gets the round's position.
//                   (A search that finds no pair has no loser: the launch then changes nothing, so the host need not know the
//                   counts before it enqueues it — one synchronisation per search, to read the two counts.)
#include <limits.h>

#include "amc_host.h"
#include "amc_philox.h"
#include "amc_cells_dev.h"

#define AMC_IC_TAG 0x414d4349u      // "AMCI": keeps these counters apart from the energised-wall draws

// two uniform doubles in [0, 1) with 53 bits each from Philox block `blk` of particle p in round `round`
__device__ inline void ic_uniform2(unsigned long long seed, unsigned int p, unsigned int blk, unsigned int round, double &u, double &v)
{
    unsigned int c[4] = {p, blk, round, AMC_IC_TAG};
    philox4x32_10(c, seed);
    u = (double)((((unsigned long long)c[0] << 32) | c[1]) >> 11) * (1.0 / 9007199254740992.0);
    v = (double)((((unsigned long long)c[2] << 32) | c[3]) >> 11) * (1.0 / 9007199254740992.0);
}

// The position of particle p in round `round` (0: amc_init_synthetic; t >= 1: the redraw of round t) from blocks 0 and 1:
// u0, u1, u2 to the cube, or to the cylinder of the region that holds index p.  u3: the block's fourth number, k_ic's.
__device__ inline void ic_position(const amc_params &P, const amc_ic_config &C, long long p, unsigned int round, double &x, double &y, double &z,
                                   double &u3)
{
    const double two_pi = 6.283185307179586;
    double u0, u1, u2;
    ic_uniform2(C.seed, (unsigned int)p, 0u, round, u0, u1);
    ic_uniform2(C.seed, (unsigned int)p, 1u, round, u2, u3);
    if (C.n_regions == 0) {
        x = u0 * P.cube_x; y = u1 * P.cube_y; z = u2 * P.cube_z;
    } else {
        int r = 0;
        while (r + 1 < C.n_regions && p >= C.first[r + 1]) r++;
        const double th = two_pi * u0, rad = C.radius[r] * sqrt(u1);
        x = rad * cos(th); y = rad * sin(th);
        z = C.z_lo[r] + (C.z_hi[r] - C.z_lo[r]) * u2;
    }
}

__global__ __launch_bounds__(256) void k_ic(amc_state S, amc_params P, amc_ic_config C, long long n)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const double two_pi = 6.283185307179586;
    double u3, u4, u5, u6, u7;
    double x, y, z;
    ic_position(P, C, p, 0u, x, y, z, u3);
    ic_uniform2(C.seed, (unsigned int)p, 2u, 0u, u4, u5);
    ic_uniform2(C.seed, (unsigned int)p, 3u, 0u, u6, u7);
    // Box-Muller on (1 - u) in (0, 1]
    const double m0 = sqrt(-2.0 * log(1.0 - u3)), m1 = sqrt(-2.0 * log(1.0 - u5));
    S.x[p] = x; S.y[p] = y; S.z[p] = z;
    S.vx[p] = C.a_shape * m0 * cos(two_pi * u4);
    S.vy[p] = C.a_shape * m0 * sin(two_pi * u4);
    S.vz[p] = C.a_shape * m1 * cos(two_pi * u6);
    S.d[p] = 0.0; S.dx[p] = 0.0; S.dy[p] = 0.0; S.dz[p] = 0.0;
    S.flag[p] = 0;
}

// what amc_init_synthetic and amc_init_separate ask of the configuration (c and cfg are not null, the struct size fits)
static int ic_config_check(amc_ctx *c, const amc_ic_config *cfg, const char *who, bool velocities)
{
    if (cfg->n_regions < 0 || cfg->n_regions > 8 || (velocities && !(cfg->a_shape >= 0.0))) return amc_fail(c, AMC_ERR_INVALID, "%s: bad configuration", who);
    if (c->n > 0xffffffffLL) return amc_fail(c, AMC_ERR_INVALID, "%s: particle index exceeds the 32-bit counter word", who);
    if (cfg->n_regions == 0 && c->P.geometry != AMC_GEOM_CUBE && c->P.geometry != AMC_GEOM_CELL)
        return amc_fail(c, AMC_ERR_INVALID, "%s: this geometry needs the region table", who);
    for (int r = 0; r < cfg->n_regions; r++)
        if (cfg->first[r] > cfg->first[r + 1] || cfg->first[0] != 0 || !(cfg->radius[r] >= 0.0) || !(cfg->z_hi[r] >= cfg->z_lo[r]))
            return amc_fail(c, AMC_ERR_INVALID, "%s: region %d is malformed", who, r);
    if (cfg->n_regions > 0 && cfg->first[cfg->n_regions] != c->n) return amc_fail(c, AMC_ERR_INVALID, "%s: the regions hold %lld particles, the context %lld", who, (long long)cfg->first[cfg->n_regions], (long long)c->n);
    return AMC_OK;
}

extern "C" int amc_init_synthetic(amc_ctx *c, const amc_ic_config *cfg)
{
    if (!c || !cfg || cfg->struct_size != (int32_t)sizeof(amc_ic_config)) return AMC_ERR_INVALID;
    if (int rc = ic_config_check(c, cfg, "amc_init_synthetic", true)) return rc;
    AMC_HIP(c, hipSetDevice(c->device));
    { int rc_ = amc_flush(c); if (rc_) return rc_; }
    c->step.lists_age = -1;          // (kept lists: a new state starts with a full build)
    amc_mg_step_fresh(c);            // (and a pending pack describes the old one)
    if (c->n > 0) {
        AMC_LAUNCH(c, k_ic, dim3((unsigned)((c->n + 255) / 256)), dim3(256), c->S, c->P, *cfg, (long long)c->n);
        AMC_HIP(c, hipGetLastError());
    }
    c->uploaded = true;
    return amc_publish_velocities(c);
}

// ---- overlap removal ---------------------------------------------------------------------------------------------------------------------
#define AMC_IC_THREADS 256
#define AMC_IC_MARK_THREADS 256
#define AMC_IC_MARK_WAVES (AMC_IC_MARK_THREADS / 64)
static_assert((long long)AMC_IC_MAX_CELLS_AXIS * AMC_IC_MAX_CELLS_AXIS * AMC_IC_MAX_CELLS_AXIS <= (1LL << 21), "cell indices fit an int with room to spare");

// the search box: n1 x n2 x n3 cells of edges w from lo, linear index (cx * n2 + cy) * n3 + cz
struct amc_ic_box {
    int n1, n2, n3, cells;
    double lo[3], w[3];
};

// cell of one coordinate, clamped into the box (below the box, or NaN: the first cell; beyond it: the last)
AMC_DEV int ic_axis(double u, double lo, double w, int n)
{
    const double f = floor((u - lo) / w);
    if (!(f >= 0.0)) return 0;
    return f >= (double)n ? n - 1 : (int)f;
}

__global__ __launch_bounds__(AMC_IC_THREADS) void k_ic_file(amc_state S, long long n, amc_ic_box B, unsigned int *cell_count, int *cell_of, int *rank_of,
                                                            unsigned char *lose)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int cx = ic_axis(amc_g(S.x)[p], B.lo[0], B.w[0], B.n1), cy = ic_axis(amc_g(S.y)[p], B.lo[1], B.w[1], B.n2),
              cz = ic_axis(amc_g(S.z)[p], B.lo[2], B.w[2], B.n3);
    const int cell = (cx * B.n2 + cy) * B.n3 + cz;
    amc_g(rank_of)[p] = (int)__hip_atomic_fetch_add(amc_g(cell_count) + cell, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    amc_g(cell_of)[p] = cell;
    amc_g(lose)[p] = 0;
}

__global__ __launch_bounds__(AMC_IC_THREADS) void k_ic_scatter(amc_state S, long long n, const unsigned int *cell_off, const int *cell_of, const int *rank_of,
                                                               int *rec_i, double *rec_s)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const size_t dst = (size_t)amc_g(cell_off)[amc_g(cell_of)[p]] + (size_t)amc_g(rank_of)[p];     // (below n: every atom is filed)
    amc_g(rec_i)[dst] = (int)p;
    auto *r = amc_g(rec_s) + dst;
    r[0] = amc_g(S.x)[p]; r[(size_t)n] = amc_g(S.y)[p]; r[2 * (size_t)n] = amc_g(S.z)[p];
}

// One home cell h (records [h0, h1)) by one wave; everything but `lane` and what is loaded per lane is wave-uniform.  Returns the
// lane's share of the pairs counted.
AMC_DEV unsigned long long ic_home(const amc_ic_box &B, int lane, int h, unsigned int h0, unsigned int h1, long long n, double md2,
                                   const unsigned int *cell_off, const int *rec_i, const double *rec_s, unsigned char *lose)
{
    const int n1 = B.n1, n2 = B.n2, n3 = B.n3;
    const int cz = h % n3, cy = (h / n3) % n2, cx = h / (n3 * n2);
    const auto *off = amc_g(cell_off);
    const auto *gi = amc_g(rec_i);
    const auto *gs = amc_g(rec_s);
    auto *gl = amc_g(lose);
    const size_t N = (size_t)n;
    unsigned long long pairs = 0;
    for (unsigned int ct = h0; ct < h1; ct += 64) {
        // the tile's centres, one per lane (a lane without one: an index no neighbour's exceeds)
        const unsigned int ci = ct + (unsigned int)lane;
        int c_idx = INT_MAX;
        double c_x = 0.0, c_y = 0.0, c_z = 0.0;
        if (ci < h1) { c_idx = gi[ci]; c_x = gs[ci]; c_y = gs[N + ci]; c_z = gs[2 * N + ci]; }
        const unsigned long long centres = __ballot(ci < h1);
        // the 3 x 3 runs of cells around the home cell, clipped at the box faces: cells adjacent along z are one run of records
        const int zl = max(cz - 1, 0), zh = min(cz + 1, n3 - 1);
        for (int X = max(cx - 1, 0); X <= min(cx + 1, n1 - 1); X++)
            for (int Y = max(cy - 1, 0); Y <= min(cy + 1, n2 - 1); Y++) {
                const int row = (X * n2 + Y) * n3;
                const unsigned int j0 = off[row + zl], j1 = off[row + zh + 1];
                for (unsigned int jb = j0; jb < j1; jb += 64) {
                    const unsigned int j = jb + (unsigned int)lane;
                    int n_idx = -1;     // (a lane without a neighbour: an index no centre's is below)
                    double n_x = 0.0, n_y = 0.0, n_z = 0.0;
                    if (j < j1) { n_idx = gi[j]; n_x = gs[j]; n_y = gs[N + j]; n_z = gs[2 * N + j]; }
                    bool lost = false;
                    for (unsigned long long m = centres; m; m &= m - 1) {
                        const int k = __builtin_amdgcn_readfirstlane(__ffsll((long long)m) - 1);
                        const int i_idx = __builtin_amdgcn_readlane(c_idx, k);
                        const double dx = pair_lane(c_x, k) - n_x, dy = pair_lane(c_y, k) - n_y, dz = pair_lane(c_z, k) - n_z;
                        const double d2 = (dx * dx + dy * dy) + dz * dz;
                        if (i_idx < n_idx && d2 < md2) { lost = true; pairs++; }
                    }
                    if (lost) gl[n_idx] = 1;
                }
            }
    }
    return pairs;
}

// chunk: consecutive cells a wave takes at a time (1 .. 64: lane b < chunk reads cell b's bounds); counts: [0] pairs, [1] losers,
// [2] the cursor — the next chunk nobody has taken yet, zero at the launch.
__global__ __launch_bounds__(AMC_IC_MARK_THREADS) void k_ic_mark(amc_ic_box B, long long n, int chunk, double md2, const unsigned int *cell_off,
                                                                 const int *rec_i, const double *rec_s, unsigned char *lose, unsigned long long *counts)
{
    __shared__ unsigned long long block_pairs;
    if (threadIdx.x == 0) block_pairs = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int ncells = B.cells;
    unsigned long long pairs = 0;
    for (;;) {
        unsigned long long take = 0;
        if (lane == 0) take = __hip_atomic_fetch_add(amc_g(counts) + 2, 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const long long base = (long long)__builtin_amdgcn_readfirstlane((int)take) * chunk;     // (at most cells + waves chunks are ever taken)
        if (base >= ncells) break;
        const int cell = (int)base + lane;
        unsigned int c0 = 0, c1 = 0;
        if (lane < chunk && cell < ncells) { c0 = amc_g(cell_off)[cell]; c1 = amc_g(cell_off)[cell + 1]; }
        for (unsigned long long live = __ballot(c1 > c0); live; live &= live - 1) {
            const int b = __builtin_amdgcn_readfirstlane(__ffsll((long long)live) - 1);
            pairs += ic_home(B, lane, (int)base + b, __builtin_amdgcn_readlane(c0, b), __builtin_amdgcn_readlane(c1, b), n, md2, cell_off, rec_i,
                             rec_s, lose);
        }
    }
    for (int d = 32; d; d >>= 1) pairs += __shfl_xor(pairs, d);
    if (lane == 0 && pairs) (void)__hip_atomic_fetch_add(&block_pairs, pairs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __syncthreads();
    if (threadIdx.x == 0 && block_pairs) (void)__hip_atomic_fetch_add(amc_g(counts), block_pairs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// apply == 0: the losers are counted and nothing else happens
__global__ __launch_bounds__(AMC_IC_THREADS) void k_ic_redraw(amc_state S, amc_params P, amc_ic_config C, long long n, unsigned int round, int apply,
                                                              const unsigned char *lose, unsigned long long *counts)
{
    __shared__ unsigned int block_losers;
    if (threadIdx.x == 0) block_losers = 0;
    __syncthreads();
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool lost = p < n && amc_g(lose)[p] != 0;
    if (lost && apply) {
        double x, y, z, u3;
        ic_position(P, C, p, round, x, y, z, u3);
        amc_g(S.x)[p] = x; amc_g(S.y)[p] = y; amc_g(S.z)[p] = z;
    }
    const unsigned long long who = __ballot(lost);
    if ((threadIdx.x & 63) == 0 && who) atomicAdd(&block_losers, (unsigned int)__popcll(who));
    __syncthreads();
    if (threadIdx.x == 0 && block_losers)
        (void)__hip_atomic_fetch_add(amc_g(counts) + 1, (unsigned long long)block_losers, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The bounding box of cfg's regions cut into cells with an edge of at least min_dist * (1 + 2^-20), at most `cap` per axis.  An
// axis without a finite positive extent, or shorter than one edge, is one cell.
static amc_ic_box ic_box(const amc_ctx *c, const amc_ic_config *cfg, double min_dist, int cap)
{
    double lo[3] = {0.0, 0.0, 0.0}, hi[3] = {c->P.cube_x, c->P.cube_y, c->P.cube_z};
    if (cfg->n_regions > 0) {
        double R = 0.0, zl = cfg->z_lo[0], zh = cfg->z_hi[0];
        for (int r = 0; r < cfg->n_regions; r++) { R = std::max(R, cfg->radius[r]); zl = std::min(zl, cfg->z_lo[r]); zh = std::max(zh, cfg->z_hi[r]); }
        lo[0] = lo[1] = -R; hi[0] = hi[1] = R; lo[2] = zl; hi[2] = zh;
    }
    amc_ic_box B;
    int n[3];
    const double edge = min_dist * (1.0 + 0x1p-20);
    for (int k = 0; k < 3; k++) {
        const double ext = hi[k] - lo[k];
        n[k] = 1;
        B.lo[k] = isfinite(lo[k]) ? lo[k] : 0.0;
        B.w[k] = 1.0;
        if (isfinite(ext) && ext > 0.0 && isfinite(lo[k])) {
            const double f = floor(ext / edge);
            n[k] = f >= (double)cap ? cap : f >= 1.0 ? (int)f : 1;
            const double w = ext / (double)n[k];
            if (w > 0.0 && isfinite(w)) B.w[k] = w; else n[k] = 1;
        }
    }
    B.n1 = n[0]; B.n2 = n[1]; B.n3 = n[2]; B.cells = n[0] * n[1] * n[2];
    return B;
}

// the work space of one call: released when the call returns, after what is in flight has finished
struct ic_workspace {
    amc_ctx *c;
    amc_alloc_group group;
    unsigned int *cell_count = nullptr, *cell_off = nullptr, *wave_sum = nullptr;
    int *cell_of = nullptr, *rank_of = nullptr, *rec_i = nullptr;
    double *rec_s = nullptr;
    unsigned char *lose = nullptr;
    unsigned long long *counts = nullptr;
    explicit ic_workspace(amc_ctx *ctx) : c(ctx), group(ctx) {}
    ~ic_workspace() { (void)hipStreamSynchronize(c->stream); }      // (then the group gives the buffers back)
    bool allocate(size_t n, size_t cells)
    {
        return dalloc(c, &cell_count, cells) == hipSuccess && dalloc(c, &cell_off, cells + 1) == hipSuccess &&
               dalloc(c, &wave_sum, (size_t)AMC_PAIR_SCAN_MAX_BLOCKS * AMC_PAIR_SCAN_WAVES) == hipSuccess && dalloc(c, &cell_of, n) == hipSuccess &&
               dalloc(c, &rank_of, n) == hipSuccess && dalloc(c, &rec_i, n) == hipSuccess && dalloc(c, &rec_s, 3 * n) == hipSuccess &&
               dalloc(c, &lose, n) == hipSuccess && dalloc(c, &counts, 3) == hipSuccess;
    }
};

// one search of the current state, and the redraw of its losers with `round` if apply; *pairs, *losers: what it found (synchronises)
static int ic_search(amc_ctx *c, const amc_ic_config *cfg, const amc_ic_box &B, const ic_workspace &W, double md2, int mark_blocks, unsigned int round,
                     bool apply, unsigned long long *pairs, unsigned long long *losers)
{
    const long long n = c->n;
    const unsigned int pblocks = (unsigned int)((n + AMC_IC_THREADS - 1) / AMC_IC_THREADS);      // (n >= 2)
    // cells a wave takes at a time: one, unless that made more than 16 takes per wave (the pair sampler's rule)
    const int chunk = (int)std::max<long long>(1, std::min<long long>(64, B.cells / ((long long)mark_blocks * AMC_IC_MARK_WAVES * 16)));
    int sblocks, seg;
    pair_scan_geometry(B.cells, &sblocks, &seg);
    AMC_HIP(c, hipMemsetAsync(W.counts, 0, 3 * sizeof(unsigned long long), c->stream));
    AMC_LAUNCH(c, k_ic_file, dim3(pblocks), dim3(AMC_IC_THREADS), c->S, n, B, W.cell_count, W.cell_of, W.rank_of, W.lose);
    AMC_HIP(c, hipGetLastError());
    AMC_LAUNCH(c, k_pair_scan_sums, dim3(sblocks), dim3(AMC_PAIR_SCAN_THREADS), (const unsigned int *)W.cell_count, W.wave_sum, B.cells, seg);
    AMC_HIP(c, hipGetLastError());
    AMC_LAUNCH(c, k_pair_scan, dim3(sblocks), dim3(AMC_PAIR_SCAN_THREADS), W.cell_count, W.cell_off, (const unsigned int *)W.wave_sum, B.cells, seg);
    AMC_HIP(c, hipGetLastError());
    AMC_LAUNCH(c, k_ic_scatter, dim3(pblocks), dim3(AMC_IC_THREADS), c->S, n, (const unsigned int *)W.cell_off, (const int *)W.cell_of,
               (const int *)W.rank_of, W.rec_i, W.rec_s);
    AMC_HIP(c, hipGetLastError());
    AMC_LAUNCH(c, k_ic_mark, dim3(mark_blocks), dim3(AMC_IC_MARK_THREADS), B, n, chunk, md2, (const unsigned int *)W.cell_off, (const int *)W.rec_i,
               (const double *)W.rec_s, W.lose, W.counts);
    AMC_HIP(c, hipGetLastError());
    AMC_LAUNCH(c, k_ic_redraw, dim3(pblocks), dim3(AMC_IC_THREADS), c->S, c->P, *cfg, n, round, apply ? 1 : 0, (const unsigned char *)W.lose, W.counts);
    AMC_HIP(c, hipGetLastError());
    unsigned long long h[2] = {0, 0};
    amc_stage st(c);
    AMC_HIP(c, st.get(h, W.counts, sizeof(h)));
    AMC_HIP(c, st.finish());
    *pairs = h[0];
    *losers = h[1];
    return AMC_OK;
}

extern "C" int amc_init_separate(amc_ctx *c, const amc_ic_config *cfg, double min_dist, int32_t first_round, int32_t max_rounds, int64_t *stats)
{
    if (!c || !cfg || cfg->struct_size != (int32_t)sizeof(amc_ic_config)) return AMC_ERR_INVALID;
    if (int rc = ic_config_check(c, cfg, "amc_init_separate", false)) return rc;
    if (!(isfinite(min_dist) && min_dist > 0.0)) return amc_fail(c, AMC_ERR_INVALID, "amc_init_separate: min_dist %g must be finite and > 0", min_dist);
    if (first_round < 1 || max_rounds < 0 || (int64_t)first_round + (int64_t)max_rounds > (int64_t)INT32_MAX)
        return amc_fail(c, AMC_ERR_INVALID, "amc_init_separate: first_round %d must be >= 1, max_rounds %d >= 0 and their sum an int32", (int)first_round,
                        (int)max_rounds);
    if (c->n > (long long)INT_MAX) return amc_fail(c, AMC_ERR_INVALID, "amc_init_separate: %lld particles (at most 2^31 - 1)", (long long)c->n);
    if (!c->uploaded) return amc_fail(c, AMC_ERR_STATE, "amc_init_separate before amc_upload / amc_init_synthetic");
    AMC_HIP(c, hipSetDevice(c->device));
    { int rc_ = amc_flush(c); if (rc_) return rc_; }
    c->step.lists_age = -1;          // (kept lists: a changed state starts with a full build)
    amc_mg_step_fresh(c);            // (and a pending pack describes the old one)
    int64_t s[AMC_IC_STATS] = {0, 0, 0, 0, 0, 0, 0, first_round};
    if (c->n >= 2) {                 // (fewer atoms have no pair: one search that finds nothing, and no launch)
        const char *env = getenv("AMC_IC_CELLS");
        const int cap = std::max(1, std::min(AMC_IC_MAX_CELLS_AXIS, env ? atoi(env) : AMC_IC_MAX_CELLS_AXIS));
        const amc_ic_box B = ic_box(c, cfg, min_dist, cap);
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess || cus < 1) cus = 256;
        const int mark_blocks = std::max(1, std::min(2 * cus, (B.cells + AMC_IC_MARK_WAVES - 1) / AMC_IC_MARK_WAVES));
        ic_workspace W(c);
        if (!W.allocate((size_t)c->n, (size_t)B.cells)) return amc_fail(c, AMC_ERR_HIP, "amc_init_separate: device allocation failed");
        AMC_HIP(c, hipMemsetAsync(W.cell_count, 0, sizeof(unsigned int) * (size_t)B.cells, c->stream));
        const double md2 = min_dist * min_dist;
        int32_t t = first_round, rounds = 0;
        for (;;) {
            const bool apply = rounds < max_rounds;
            unsigned long long pairs, losers;
            if (int rc = ic_search(c, cfg, B, W, md2, mark_blocks, (unsigned int)t, apply, &pairs, &losers)) return rc;
            if (s[0] == 0) { s[3] = (int64_t)pairs; s[4] = (int64_t)losers; }
            s[0]++;
            s[5] = (int64_t)pairs; s[6] = (int64_t)losers;
            if (pairs == 0 || !apply) break;
            s[2] += (int64_t)losers;
            t++; rounds++;
        }
        s[1] = rounds;
        s[7] = t;
    } else {
        s[0] = 1;
    }
    if (stats) memcpy(stats, s, sizeof(s));
    return AMC_OK;
}
