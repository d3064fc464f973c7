// amc_surface.hip — sampled surfaces: per energised case (3..9) and wall bin, the number of hits and the z-momentum and energy
// the gas exchanged there, accumulated as exact integers (include/argonmc.h "sampled surfaces").  The reference
// reports three sums per step (Temp:756-758); the Python layer derives rates per area from the totals.
//
// The data is already on the device: every hit of cases 3..9 leaves a record (particle, contact point, ok, dp_z, dE) — in the
// segments of the device-RNG mode, or in the hand-over's records plus what its apply kernels write.  k_surface_accum is ONE
// workgroup: it strides over the records it is given, computes the bin and the two quantised values of each in registers and
// adds them into a table in LDS (64-bit integer LDS atomics: exact and order-free); after a barrier the thread that owns a column
// adds it into the 128-bit running totals with carry.  A single workgroup owns the totals: no global atomics.  None of the
// step's own kernels is involved: the launch sits behind the kernel that completes the records and in front of whatever
// clears or overwrites them (stream order).
#include "amc_case_sums_dev.h"
#include "amc_host.h"
#include "amc_sample_dev.h"

#define AMC_SURFACE_Q 3                 // count, q(dp_z), q(dE)
#define AMC_SURFACE_THREADS 1024
#define AMC_SURFACE_COLUMNS (AMC_SURFACE_CASES * (AMC_SURFACE_MAX_BINS + 1) * AMC_SURFACE_Q)      // 5,397 x 8 B = 42.2 KiB
#define AMC_SURFACE_PER_THREAD ((AMC_SURFACE_COLUMNS + AMC_SURFACE_THREADS - 1) / AMC_SURFACE_THREADS)   // columns of the totals a thread owns: 6

#define AMC_SURFACE_MAX_PARTICLES (1LL << 24)    // the record capacities are N / 64 + 1,024 per case (device RNG), N / 8 + 1,024 (hand-over): < 2^22 per launch
#define AMC_SURFACE_ACCUM 0             // records with contact point and results: bin and add
#define AMC_SURFACE_BIN 1               // a case being parked: bin of every record -> park_bin (its results come later)
#define AMC_SURFACE_FINISH 2            // ... and its results into those bins

struct amc_surface_grid_dev {
    int nbins;
    double lo[AMC_SURFACE_CASES], hi[AMC_SURFACE_CASES], w[AMC_SURFACE_CASES];
};

// the records of nseg cases, case 3 + first + k at offset k * stride
struct amc_surface_src {
    const int *idx;
    const double *contact;              // [3 * records]
    const unsigned char *ok;
    const double *dpz, *dE;
    const int *count;                   // records per case as the device counted them ([first + k]; clamped to cap), or
    int n;                              // (count == nullptr) the one case's records as the host knows them
    int cap;                            // records a case has room for
    int first, nseg;
    size_t stride;
};

// bin of a coordinate: nbins = outside (below lo, beyond hi, NaN); u == hi lands in the last bin
AMC_DEV int amc_surface_bin(double u, double lo, double hi, double w, int n)
{
    const int b = amc_fields_axis(u, lo, hi, w, n);
    return b < 0 ? n : b;
}

// The kernel is a chain of memory round trips for a few hundred records, not bandwidth: whatever does not depend on anything
// else — the error word, the record counts, this thread's columns of the totals — is loaded side by side at the start, and a
// record's fields are all loaded before the first of them is looked at.  One round trip for those, one for the records
// (1,024 threads: a step at N = 1e6 has about 600), stores at the end.
template <int MODE>
__global__ __launch_bounds__(AMC_SURFACE_THREADS) void k_surface_accum(amc_surface_src R, amc_surface_grid_dev G,
                                                                       int *__restrict__ park_bin, unsigned long long *__restrict__ tot,
                                                                       unsigned long long *__restrict__ meta)
{
    __shared__ unsigned long long tab[AMC_SURFACE_COLUMNS];
    __shared__ unsigned int s_failed[AMC_SURFACE_CASES];
    __shared__ int s_n[AMC_SURFACE_CASES];
    __shared__ unsigned int s_bad;
    const int tid = threadIdx.x;
    const int nb1 = G.nbins + 1, M = AMC_SURFACE_CASES * nb1 * AMC_SURFACE_Q;
    const unsigned long long bad0 = meta[0];
    unsigned long long failed0 = 0;
    int cnt = 0;
    if (tid < AMC_SURFACE_CASES) failed0 = meta[1 + tid];
    if (tid < R.nseg) cnt = R.count ? R.count[R.first + tid] : R.n;
    ulonglong2 t0[AMC_SURFACE_PER_THREAD];
#pragma unroll
    for (int i = 0; i < AMC_SURFACE_PER_THREAD; i++) {
        const int j = tid + i * AMC_SURFACE_THREADS;
        t0[i] = j < M ? ((const ulonglong2 *)tot)[j] : make_ulonglong2(0, 0);
    }
    for (int j = tid; j < M; j += AMC_SURFACE_THREADS) tab[j] = 0;
    if (tid < AMC_SURFACE_CASES) {
        s_failed[tid] = 0;
        s_n[tid] = amc_clamp_count(cnt, R.cap);
    }
    if (tid == 0) s_bad = ~0u;
    __syncthreads();
    if (bad0 != ~0ULL) return;          // a hit out of range has stopped the accumulation (amc_surface_read reports it)
    constexpr bool finish = MODE == AMC_SURFACE_FINISH, bin_only = MODE == AMC_SURFACE_BIN;
    for (int seg = 0; seg < R.nseg; seg++) {
        const int s = R.first + seg, n = s_n[seg];
        const size_t off = (size_t)seg * R.stride;
        const bool plane = s == 0 || s == 1 || s == 3 || s == 4;       // cases 3, 4, 6, 7
        for (int k = tid; k < n; k += AMC_SURFACE_THREADS) {
            const size_t o = off + (size_t)k;
            int bin = 0, particle = 0;
            unsigned char ok = 1;
            double cx = 0, cy = 0, cz = 0, dpz = 0, dE = 0;
            if (finish) bin = park_bin[k];
            else { ok = R.ok[o]; cx = R.contact[3 * o]; cy = R.contact[3 * o + 1]; cz = R.contact[3 * o + 2]; }
            if (!bin_only) { dpz = R.dpz[o]; dE = R.dE[o]; particle = R.idx[o]; }
            if (finish) {
                if (bin < 0 || bin > G.nbins) continue;                 // (a failed contact solve: counted when the case was parked)
            } else {
                if (!ok) {
                    atomicAdd(&s_failed[s], 1u);
                    if (bin_only) park_bin[k] = -1;
                    continue;
                }
                const double u = plane ? sqrt(cx * cx + cy * cy) : cz;
                bin = amc_surface_bin(u, G.lo[s], G.hi[s], G.w[s], G.nbins);
                if (bin_only) { park_bin[k] = bin; continue; }
            }
            if (!(fabs(dpz) < 0x1p-70) || !(fabs(dE) < 0x1p-57)) { atomicMin(&s_bad, (unsigned int)particle); continue; }
            unsigned long long *t = tab + (size_t)(s * nb1 + bin) * AMC_SURFACE_Q;
            atomicAdd(t + 0, 1ULL);
            atomicAdd(t + 1, (unsigned long long)(long long)rint(ldexp(dpz, 110)));
            atomicAdd(t + 2, (unsigned long long)(long long)rint(ldexp(dE, 97)));
        }
    }
    __syncthreads();
    if (s_bad != ~0u) {                 // this launch adds nothing, and no later one does
        if (tid == 0) meta[0] = (unsigned long long)s_bad;
        return;
    }
    if (tid < AMC_SURFACE_CASES && s_failed[tid]) meta[1 + tid] = failed0 + (unsigned long long)s_failed[tid];
#pragma unroll
    for (int i = 0; i < AMC_SURFACE_PER_THREAD; i++) {
        const int j = tid + i * AMC_SURFACE_THREADS;
        if (j >= M) break;
        const unsigned long long a = tab[j];        // (wraps modulo 2^64; the true sum of one launch is at most 2^62 in magnitude)
        if (!a) continue;
        ulonglong2 v = t0[i];
        amc_add128(v.x, v.y, a);
        ((ulonglong2 *)tot)[j] = v;
    }
}

static hipError_t surface_launch(amc_ctx *c, const amc_surface_src &R, int mode)
{
    const amc_surface_ws &F = c->SF;
    amc_surface_grid_dev G;
    G.nbins = F.g.nbins;
    for (int s = 0; s < AMC_SURFACE_CASES; s++) { G.lo[s] = F.g.lo[s]; G.hi[s] = F.g.hi[s]; G.w[s] = F.w[s]; }
    amc_prof_begin(c, AMC_K_FIELDS);
    if (mode == AMC_SURFACE_ACCUM)
        AMC_LAUNCH(c, k_surface_accum<AMC_SURFACE_ACCUM>, dim3(1), dim3(AMC_SURFACE_THREADS), R, G, F.park_bin, F.tot, F.meta);
    else if (mode == AMC_SURFACE_BIN)
        AMC_LAUNCH(c, k_surface_accum<AMC_SURFACE_BIN>, dim3(1), dim3(AMC_SURFACE_THREADS), R, G, F.park_bin, F.tot, F.meta);
    else
        AMC_LAUNCH(c, k_surface_accum<AMC_SURFACE_FINISH>, dim3(1), dim3(AMC_SURFACE_THREADS), R, G, F.park_bin, F.tot, F.meta);
    amc_prof_end(c);
    return hipGetLastError();
}

hipError_t amc_launch_surface_device(amc_ctx *c)
{
    const temp_dev_segments &D = c->TD.seg;
    amc_surface_src R;
    R.idx = D.idx; R.contact = D.contact; R.ok = D.ok; R.dpz = D.dpz; R.dE = D.dE;
    R.count = D.count; R.n = 0; R.cap = D.cap; R.first = 0; R.nseg = AMC_SURFACE_CASES; R.stride = (size_t)D.cap;
    return surface_launch(c, R, AMC_SURFACE_ACCUM);
}

// the hand-over's current case: its n records (n <= T.cap: amc_wall_hits) and what k_temp_apply wrote for them
static amc_surface_src surface_case_src(amc_ctx *c, int case_id, int n)
{
    const amc_temp_ws &T = c->T;
    amc_surface_src R;
    R.idx = T.idx; R.contact = T.contact; R.ok = T.ok; R.dpz = T.dpz; R.dE = T.dE;
    R.count = nullptr; R.n = n; R.cap = T.cap; R.first = case_id - 3; R.nseg = 1; R.stride = 0;
    return R;
}

hipError_t amc_launch_surface_case(amc_ctx *c, int case_id, int n)
{
    if (n <= 0) return hipSuccess;
    return surface_launch(c, surface_case_src(c, case_id, n), AMC_SURFACE_ACCUM);
}

// A parked case in two launches: the next case's k_temp_hits, launched ahead, overwrites the contact points before the
// results exist.  The bins are computed now and kept per record; amc_launch_surface_finish adds def_dpz / def_dE into them.
int amc_surface_park(amc_ctx *c, int case_id, int n)
{
    amc_surface_ws &F = c->SF;
    F.park_case = 0;
    if (n <= 0) return AMC_OK;
    if (!F.park_bin) AMC_HIP(c, dalloc(c, &F.park_bin, (size_t)c->T.cap));
    AMC_HIP(c, surface_launch(c, surface_case_src(c, case_id, n), AMC_SURFACE_BIN));
    F.park_case = case_id; F.park_n = n;
    return AMC_OK;
}

hipError_t amc_launch_surface_finish(amc_ctx *c, int case_id, int n)
{
    amc_surface_ws &F = c->SF;
    const bool mine = F.park_case == case_id && F.park_n == n && n > 0;    // (else: the grid was configured after the park)
    F.park_case = 0;
    if (!mine) return hipSuccess;
    const amc_temp_ws &T = c->T;
    amc_surface_src R = surface_case_src(c, case_id, n);
    R.idx = T.def_idx; R.contact = nullptr; R.ok = nullptr; R.dpz = T.def_dpz; R.dE = T.def_dE;
    return surface_launch(c, R, AMC_SURFACE_FINISH);
}

// meta: [0] the error word, [1 + s] failed contact solves of case 3 + s
static amc_totals surface_totals(const amc_surface_ws &F)
{
    return amc_totals{F.tot, (size_t)2 * AMC_SURFACE_Q * AMC_SURFACE_CASES * (size_t)(F.g.nbins + 1), F.meta, 1 + AMC_SURFACE_CASES, 0};
}

static void surface_free(amc_ctx *c)
{
    ctx_free(c, c->SF.tot, c->SF.meta, c->SF.park_bin);
    c->SF = amc_surface_ws();
}

// totals (zero when nullptr), the per-case failed solves (likewise), no hit out of range
static int surface_put(amc_ctx *c, const int64_t *totals, const int64_t *n_failed)
{
    amc_surface_ws &F = c->SF;
    unsigned long long meta[1 + AMC_SURFACE_CASES] = {0};
    for (int s = 0; s < AMC_SURFACE_CASES; s++) meta[1 + s] = n_failed ? (unsigned long long)n_failed[s] : 0ULL;
    if (int rc = amc_totals_put(c, surface_totals(F), totals, meta)) return rc;
    F.lost = false;
    F.park_case = 0;            // (a case parked before the totals were replaced finishes without adding to them)
    return AMC_OK;
}

// what the sampler asks of the context
static int surface_needs(amc_ctx *c)
{
    if (c->P.geometry != AMC_GEOM_PORE_ENERGISED) return amc_fail(c, AMC_ERR_STATE, "amc_surface_config needs AMC_GEOM_PORE_ENERGISED");
    if (c->n > AMC_SURFACE_MAX_PARTICLES)
        return amc_fail(c, AMC_ERR_CAPACITY, "amc_surface_config: %lld particles (at most 2^24 keep a launch below 2^22 hit records and its sums exact)", (long long)c->n);
    return AMC_OK;
}

extern "C" {

int amc_surface_config(amc_ctx *c, const amc_surface_grid *g)
{
    bool done;
    if (int rc = amc_sampler_config_begin(c, g, "amc_surface_grid", surface_free, &done, surface_needs); rc || done) return rc;
    if (g->nbins < 1 || g->nbins > AMC_SURFACE_MAX_BINS)
        return amc_fail(c, AMC_ERR_INVALID, "amc_surface_grid: %d bins (1 .. %d)", g->nbins, AMC_SURFACE_MAX_BINS);
    for (int s = 0; s < AMC_SURFACE_CASES; s++)
        if (!(isfinite(g->lo[s]) && isfinite(g->hi[s]) && g->lo[s] < g->hi[s]))
            return amc_fail(c, AMC_ERR_INVALID, "amc_surface_grid: case %d needs finite bounds lo < hi", 3 + s);
    surface_free(c);
    amc_surface_ws &F = c->SF;
    F.g = *g;
    for (int s = 0; s < AMC_SURFACE_CASES; s++) F.w[s] = (g->hi[s] - g->lo[s]) / (double)g->nbins;
    if (dalloc(c, &F.tot, surface_totals(F).words) != hipSuccess || dalloc(c, &F.meta, 1 + AMC_SURFACE_CASES) != hipSuccess) {
        surface_free(c);
        return amc_fail(c, AMC_ERR_HIP, "amc_surface_config: device allocation failed");
    }
    F.on = true;
    if (int rc = surface_put(c, nullptr, nullptr)) { surface_free(c); return rc; }
    return AMC_OK;
}

int amc_surface_read(amc_ctx *c, int64_t *totals, int64_t *n_failed, int64_t *n_steps)
{
    if (!c) return AMC_ERR_INVALID;
    amc_surface_ws &F = c->SF;
    if (!F.on) return amc_fail(c, AMC_ERR_STATE, "amc_surface_read before amc_surface_config");
    if (F.lost)
        return amc_fail(c, AMC_ERR_STATE, "amc_surface_read: a step overflowed its hit records or work buffers (AMC_ERR_CAPACITY), hits are "
                        "missing from the totals; amc_surface_reset, amc_surface_load or amc_surface_config start again");
    AMC_HIP(c, hipSetDevice(c->device));
    unsigned long long meta[1 + AMC_SURFACE_CASES], bad;
    if (int rc = amc_totals_get(c, surface_totals(F), totals, meta, &bad)) return rc;
    if (bad != ~0ULL)
        return amc_fail(c, AMC_ERR_CAPACITY, "amc_surface: the hit of particle %llu is outside |dpz| < 2^-70 kg m/s, |dE| < 2^-57 J (or NaN); "
                        "sampling stopped until amc_surface_reset", bad);
    for (int s = 0; s < AMC_SURFACE_CASES && n_failed; s++) n_failed[s] = (int64_t)meta[1 + s];
    if (n_steps) *n_steps = F.n_steps;
    return AMC_OK;
}

int amc_surface_load(amc_ctx *c, const int64_t *totals, const int64_t *n_failed, int64_t n_steps)
{
    if (!c || !totals || !n_failed || n_steps < 0) return AMC_ERR_INVALID;
    for (int s = 0; s < AMC_SURFACE_CASES; s++)
        if (n_failed[s] < 0) return AMC_ERR_INVALID;
    if (!c->SF.on) return amc_fail(c, AMC_ERR_STATE, "amc_surface_load before amc_surface_config");
    AMC_HIP(c, hipSetDevice(c->device));
    if (int rc = surface_put(c, totals, n_failed)) return rc;
    c->SF.n_steps = n_steps;
    return AMC_OK;
}

int amc_surface_reset(amc_ctx *c)
{
    if (!c) return AMC_ERR_INVALID;
    if (int rc = amc_sampler_ready(c, c->SF.on, "amc_surface", "reset")) return rc;
    if (int rc = surface_put(c, nullptr, nullptr)) return rc;
    c->SF.n_steps = 0;
    return AMC_OK;
}

}  // extern "C"
