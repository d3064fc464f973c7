// amc_mfp.hip — sampled free paths: per spatial bin and ending kind (a wall, another atom) the number of completed free paths,
// the sums of their four lengths and of the total's square, and a histogram of the total, accumulated as exact integers
// (include/argonmc_mfp.h).  The reference reports four global histograms; the Python layer derives the local
// mean free path, the wall's share and the rate of path ends per volume from the totals.
//
// The data is already on the device: every completed path leaves a record (amc_emit), and the owner's final position is in the
// particle arrays or, where the last sweep left its results pending, in the slot arrays.  k_mfp_accum is ONE workgroup, like
// k_surface_accum: it strides over the records behind its cursor, computes bin, kind and the quantised values of each in
// registers and adds them into a table in LDS (64-bit integer LDS atomics: exact and order-free); after a barrier the thread
// that owns a column adds it into the running totals, the 128-bit ones with carry.  A single workgroup owns the totals: no
// global atomics.  None of the step's own kernels is involved: the launch sits behind the kernel that completes the step's
// records (the commit) and in front of whatever emits the next step's (stream order).
#include "amc_host.h"
#include "amc_sample_dev.h"
#include <cstddef>

#define AMC_MFP_Q AMC_SAMPLE_Q          // count, q(total), q(px), q(py), q(pz), q(total * total), reserved
#define AMC_MFP_THREADS 1024
#define AMC_MFP_PER_THREAD (AMC_MFP_MAX_COLUMNS / AMC_MFP_THREADS)      // columns of the table a thread owns: 6
#define AMC_MFP_MAX_RECORDS (1u << 22)  // per launch: 2^22 values of at most 2^40 stay below 2^62
#define AMC_MFP_MAX_PARTICLES (1LL << 24)
#define AMC_MFP_NMETA 5
static_assert(AMC_MFP_MAX_COLUMNS % AMC_MFP_THREADS == 0, "every thread owns the same number of columns");
static_assert(sizeof(amc_path_record) == 64 && offsetof(amc_path_record, phase) == 4 && offsetof(amc_path_record, i) == 16 &&
              offsetof(amc_path_record, which) == 24 && offsetof(amc_path_record, total) == 32 && offsetof(amc_path_record, pz) == 56,
              "a record is four 16-byte pieces: step phase cell | i j which - | total px | py pz");

// a 16-byte piece of a record (four to a record), as a plain vector: a value in registers, not a structure
typedef unsigned int mfp_piece __attribute__((ext_vector_type(4)));
AMC_DEV double mfp_f64(unsigned int lo, unsigned int hi) { return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo)); }

struct amc_mfp_args {
    const amc_path_record *rec;
    unsigned int *path_count;
    unsigned int cap;
    int consume;                        // keep_records == 0: the launch empties the record buffer
    long long n;                        // particles: an owner outside [0, n) is reported, not looked up
    const double *x, *y, *z;
    amc_lazy L;
    amc_fields_grid_dev G;
    int hist_bins;
    double hist_hi, hist_w;
    unsigned long long *tot, *hist, *meta;
};

// The kernel is a chain of memory round trips for a few thousand records (a step of the pore at N = 1e6 completes about 2,500
// paths, one of the cube at N = 1e5 about 400), not bandwidth: one trip for what depends on nothing (the error word, the cursor,
// path_count, this thread's columns of the totals), then per pass of 1,024 records two to four dependent ones, stores at the
// end.
__global__ __launch_bounds__(AMC_MFP_THREADS) void k_mfp_accum(amc_mfp_args A)
{
    __shared__ unsigned long long tab[AMC_MFP_MAX_COLUMNS];     // 48 KiB
    __shared__ mfp_piece stage[AMC_MFP_THREADS / 64][64 * 4];   // 64 KiB: the 64 records a wave is working on, as it loaded them
    __shared__ unsigned int s_bad, s_outside, s_binned;
    const int tid = threadIdx.x;
    const int C = AMC_MFP_Q + A.hist_bins + 1;          // columns per (bin, kind): the seven sums, the histogram, "beyond"
    const int M = A.G.bins * 2 * C;
    auto *meta = amc_g(A.meta);
    ulonglong2 *tot = (ulonglong2 *)A.tot;        // (whole (low, high) pairs: moved through amc_g_load / amc_g_store)
    auto *hist = amc_g(A.hist);
    const unsigned long long bad0 = meta[0], cursor0 = meta[3], lost0 = meta[4];
    const unsigned int pc = *amc_g(A.path_count);
    unsigned long long n_rec0 = 0, n_out0 = 0;
    if (tid == 0) { n_rec0 = meta[1]; n_out0 = meta[2]; }
    ulonglong2 t0[AMC_MFP_PER_THREAD];
#pragma unroll
    for (int i = 0; i < AMC_MFP_PER_THREAD; i++) {
        const int j = tid + i * AMC_MFP_THREADS;
        t0[i] = make_ulonglong2(0, 0);
        if (j < M) {
            const int bk = j / C, q = j - bk * C;
            if (q < AMC_MFP_Q) t0[i] = amc_g_load(tot + (bk * AMC_MFP_Q + q));
            else t0[i].x = hist[bk * (C - AMC_MFP_Q) + (q - AMC_MFP_Q)];
        }
    }
    for (int j = tid; j < M; j += AMC_MFP_THREADS) tab[j] = 0;
    if (tid == 0) { s_bad = ~0u; s_outside = 0; s_binned = 0; }
    __syncthreads();
    // the records this launch sees: [cursor, end).  path_count above the capacity, a cursor beyond the end or more unseen records
    // than one launch can sum: records are missing, the totals are marked lost
    const unsigned int end = pc < A.cap ? pc : A.cap;
    const bool lost = pc > A.cap || cursor0 > (unsigned long long)end || (unsigned long long)end - cursor0 > AMC_MFP_MAX_RECORDS;
    if (tid == 0) {                     // the records count as seen whatever becomes of them
        meta[3] = A.consume ? 0ULL : (unsigned long long)end;
        if (A.consume) *amc_g(A.path_count) = 0u;
        if (lost && !lost0) meta[4] = 1ULL;
    }
    if (bad0 != ~0ULL || lost0 || lost) return;         // (amc_mfp_read reports either; nothing is added until a reset)
    unsigned int outside = 0, binned = 0;
    // A wave's 64 records are 4 KiB in a row: it loads them as 256 pieces of 16 bytes, lane after lane — 64 cache lines instead of
    // the 256 that 64 lanes reading one record each would touch: the kernel runs on ONE CU, and what it costs per record is that CU's
    // rate of cache-line accesses — and every lane takes its own record out of LDS.
    const int lane = tid & 63, wave = tid >> 6;
    for (unsigned int kb = (unsigned int)cursor0 + (unsigned int)(wave * 64); kb < end; kb += AMC_MFP_THREADS) {
        const unsigned int left = end - kb;             // records of this wave's block that exist (>= 1)
        __builtin_amdgcn_wave_barrier();                // (the lanes have taken the last block's records)
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int piece = c * 64 + lane;
            if ((unsigned int)(piece >> 2) < left) stage[wave][piece] = *((const AMC_AS_GLOBAL mfp_piece *)(A.rec + kb) + piece);
        }
        __builtin_amdgcn_wave_barrier();                // (LDS serves a wave's accesses in order: the reads below see the stores)
        if ((unsigned int)lane >= left) continue;
        const mfp_piece p0 = stage[wave][lane * 4], p1 = stage[wave][lane * 4 + 1], p2 = stage[wave][lane * 4 + 2], p3 = stage[wave][lane * 4 + 3];
        const int phase = (int)p0.y, ri = (int)p1.x, rj = (int)p1.y, which = (int)p1.z;       // step phase cell | i j which -
        const double v[4] = {mfp_f64(p2.x, p2.y), mfp_f64(p2.z, p2.w), mfp_f64(p3.x, p3.y), mfp_f64(p3.z, p3.w)};       // total px | py pz
        const bool pp = phase >= 16;
        const int owner = pp ? (which ? ri : rj) : ri;
        if (owner < 0 || (long long)owner >= A.n) { atomicMin(&s_bad, owner < 0 ? 0xfffffffeu : (unsigned int)owner); continue; }
        double x = amc_g(A.x)[owner], y = amc_g(A.y)[owner], z = amc_g(A.z)[owner];
        double vx, vy, vz;              // (not looked at: their loads fall away)
        amc_fields_lazy(A.L, owner, x, y, z, vx, vy, vz);
        const int bin = amc_sample_bin(A.G, x, y, z);
        if (bin < 0) { outside++; continue; }
        bool ok = true;
#pragma unroll
        for (int e = 0; e < 4; e++) ok = ok && v[e] >= 0.0 && v[e] < 0x1p-16;     // (false for NaN)
        if (!ok) { atomicMin(&s_bad, (unsigned int)owner); continue; }
        unsigned long long *t = tab + (size_t)(bin * 2 + (pp ? 1 : 0)) * C;
        atomicAdd(t + 0, 1ULL);
#pragma unroll
        for (int e = 0; e < 4; e++) atomicAdd(t + 1 + e, (unsigned long long)(long long)rint(ldexp(v[e], 56)));
        atomicAdd(t + 5, (unsigned long long)(long long)rint(ldexp(v[0] * v[0], 72)));
        if (A.hist_bins > 0) {
            int h = v[0] < A.hist_hi ? amc_fields_axis(v[0], 0.0, A.hist_hi, A.hist_w, A.hist_bins) : -1;
            if (h < 0) h = A.hist_bins;
            atomicAdd(t + AMC_MFP_Q + h, 1ULL);
        }
        binned++;
    }
    if (outside) atomicAdd(&s_outside, outside);
    if (binned) atomicAdd(&s_binned, binned);
    __syncthreads();
    if (s_bad != ~0u) {                 // this launch adds nothing, and no later one does
        if (tid == 0) meta[0] = (unsigned long long)s_bad;
        return;
    }
    if (tid == 0) {
        if (s_binned) meta[1] = n_rec0 + (unsigned long long)s_binned;
        if (s_outside) meta[2] = n_out0 + (unsigned long long)s_outside;
    }
#pragma unroll
    for (int i = 0; i < AMC_MFP_PER_THREAD; i++) {
        const int j = tid + i * AMC_MFP_THREADS;
        if (j >= M) break;
        const unsigned long long a = tab[j];            // (at most 2^62: no wrap)
        if (!a) continue;
        const int bk = j / C, q = j - bk * C;
        ulonglong2 v = t0[i];
        if (q < AMC_MFP_Q) {
            amc_add128(v.x, v.y, a);
            amc_g_store(tot + (bk * AMC_MFP_Q + q), v);
        } else {
            hist[bk * (C - AMC_MFP_Q) + (q - AMC_MFP_Q)] = v.x + a;
        }
    }
}

// meta: [0] the error word, [1] records binned, [2] owners outside, [3] the cursor, [4] lost
static amc_totals mfp_totals(const amc_mfp_ws &F)
{
    return amc_totals{F.tot, (size_t)2 * AMC_MFP_Q * 2 * (size_t)F.G.bins, F.meta, AMC_MFP_NMETA, 0};
}
static size_t mfp_hist_words(const amc_mfp_ws &F) { return (size_t)F.G.bins * 2 * (size_t)(F.g.hist_bins + 1); }

static void mfp_free(amc_ctx *c)
{
    ctx_free(c, c->MF.tot, c->MF.hist, c->MF.meta);
    c->MF = amc_mfp_ws();
}

// totals and histograms (zero when nullptr), the two counters, no error, nothing lost; the cursor stays where it is
static int mfp_put(amc_ctx *c, const int64_t *totals, const int64_t *hist, int64_t n_records, int64_t n_outside)
{
    amc_mfp_ws &F = c->MF;
    unsigned long long cursor = 0;
    AMC_HIP(c, hipMemcpyAsync(&cursor, F.meta + 3, sizeof cursor, hipMemcpyDeviceToHost, c->stream));
    AMC_HIP(c, hipStreamSynchronize(c->stream));
    const unsigned long long meta[AMC_MFP_NMETA] = {0, (unsigned long long)n_records, (unsigned long long)n_outside, cursor, 0};
    if (hist) AMC_HIP(c, hipMemcpyAsync(F.hist, hist, sizeof(unsigned long long) * mfp_hist_words(F), hipMemcpyHostToDevice, c->stream));
    else AMC_HIP(c, hipMemsetAsync(F.hist, 0, sizeof(unsigned long long) * mfp_hist_words(F), c->stream));
    if (int rc = amc_totals_put(c, mfp_totals(F), totals, meta)) return rc;
    F.lost = false;
    return AMC_OK;
}

// what the sampler asks of the context
static int mfp_needs(amc_ctx *c)
{
    if (!c->d_rec) return amc_fail(c, AMC_ERR_STATE, "amc_mfp_config needs path records (amc_params.max_paths >= 0)");
    if (c->n > AMC_MFP_MAX_PARTICLES)
        return amc_fail(c, AMC_ERR_CAPACITY, "amc_mfp_config: %lld particles (at most 2^24, as for the other samplers)", (long long)c->n);
    return AMC_OK;
}

extern "C" {

int amc_mfp_step(amc_ctx *c)
{
    amc_mfp_ws &F = c->MF;
    // the cube's p-p paths otherwise wait for the next streaming pass: the step's records are complete behind its commit
    if (int rc = amc_settle_commit(c)) return rc;
    amc_mfp_args A;
    A.rec = c->d_rec; A.path_count = &c->d_cnt->path_count; A.cap = c->out.cap; A.consume = F.g.keep_records ? 0 : 1;
    A.n = (long long)c->n; A.x = c->S.x; A.y = c->S.y; A.z = c->S.z;
    A.L = amc_sample_lazy(c);
    A.G = F.G; A.hist_bins = F.g.hist_bins; A.hist_hi = F.g.hist_hi; A.hist_w = F.hist_w;
    A.tot = F.tot; A.hist = F.hist; A.meta = F.meta;
    amc_prof_begin(c, AMC_K_FIELDS);
    AMC_LAUNCH(c, k_mfp_accum, dim3(1), dim3(AMC_MFP_THREADS), A);
    amc_prof_end(c);
    AMC_HIP(c, hipGetLastError());
    F.n_steps++;
    return AMC_OK;
}

int amc_mfp_rewind(amc_ctx *c)
{
    AMC_HIP(c, hipMemsetAsync(c->MF.meta + 3, 0, sizeof(unsigned long long), c->stream));
    return AMC_OK;
}

int amc_mfp_config(amc_ctx *c, const amc_mfp_grid *g)
{
    bool done;
    if (int rc = amc_sampler_config_begin(c, g, "amc_mfp_grid", mfp_free, &done, mfp_needs); rc || done) return rc;
    const char *fault = nullptr;
    if (g->hist_bins < 0 || g->hist_bins > AMC_MFP_MAX_HIST_BINS) fault = "hist_bins must be 0 .. 64";
    else if (g->keep_records != 0 && g->keep_records != 1) fault = "keep_records must be 0 or 1";
    else if (g->hist_bins > 0 && !(isfinite(g->hist_hi) && g->hist_hi > 0.0)) fault = "hist_hi must be finite and > 0";
    const int per_bin = 2 * (AMC_MFP_Q + (fault ? 0 : g->hist_bins) + 1);
    amc_fields_grid_dev G;
    if (int rc = amc_sample_grid_check(c, "amc_mfp_grid", "bins (2 x (7 + hist_bins + 1) columns each, 6,144 columns in all)", g->kind, g->n1, g->n2, g->n3,
                                       AMC_MFP_MAX_COLUMNS / per_bin, g->lo, g->hi, 0, 0, g->reserved == 0, fault, &G))
        return rc;
    mfp_free(c);
    amc_mfp_ws &F = c->MF;
    F.g = *g;
    F.G = G;
    F.hist_w = g->hist_bins > 0 ? g->hist_hi / (double)g->hist_bins : 1.0;
    if (dalloc(c, &F.tot, mfp_totals(F).words) != hipSuccess || dalloc(c, &F.hist, mfp_hist_words(F)) != hipSuccess ||
        dalloc(c, &F.meta, AMC_MFP_NMETA) != hipSuccess) {
        mfp_free(c);
        return amc_fail(c, AMC_ERR_HIP, "amc_mfp_config: device allocation failed");
    }
    // Paths completed before this call are not binned (a pending commit's belong to a step before it).  A consuming sampler
    // starts by emptying the record buffer, as it will after every step — also one that overflowed in a long run nobody
    // drained; with keep_records the cursor starts at the records' current end, and an overflowed buffer has to be drained first
    // (the first step marks the totals lost otherwise: path_count stays above the capacity).
    int rc = amc_settle_commit(c);
    if (!rc) {
        hipError_t e = hipMemsetAsync(F.meta, 0, sizeof(unsigned long long) * AMC_MFP_NMETA, c->stream);
        if (e == hipSuccess && !g->keep_records) e = hipMemsetAsync(&c->d_cnt->path_count, 0, sizeof(unsigned int), c->stream);
        if (e == hipSuccess && g->keep_records)
            e = hipMemcpyAsync(F.meta + 3, &c->d_cnt->path_count, sizeof(unsigned int), hipMemcpyDeviceToDevice, c->stream);
        if (e != hipSuccess) rc = amc_fail(c, AMC_ERR_HIP, "amc_mfp_config: %s", hipGetErrorString(e));
    }
    F.on = true;
    if (!rc) rc = mfp_put(c, nullptr, nullptr, 0, 0);
    if (rc) { mfp_free(c); return rc; }
    return AMC_OK;
}

int amc_mfp_read(amc_ctx *c, int64_t *totals, int64_t *hist, int64_t *n_records, int64_t *n_outside, int64_t *n_steps)
{
    if (!c) return AMC_ERR_INVALID;
    amc_mfp_ws &F = c->MF;
    if (!F.on) return amc_fail(c, AMC_ERR_STATE, "amc_mfp_read before amc_mfp_config");
    static const char *lost = "amc_mfp_read: path records were lost (the record buffer overflowed, a step left more than 2^22 unseen records, or an "
                              "energised step returned AMC_ERR_CAPACITY), paths are missing from the totals; amc_mfp_reset, amc_mfp_load or "
                              "amc_mfp_config start again";
    if (F.lost) return amc_fail(c, AMC_ERR_STATE, "%s", lost);
    AMC_HIP(c, hipSetDevice(c->device));
    unsigned long long meta[AMC_MFP_NMETA], bad;
    amc_stage st(c);
    if (hist) AMC_HIP(c, st.get(hist, F.hist, sizeof(unsigned long long) * mfp_hist_words(F)));
    if (totals) AMC_HIP(c, st.get(totals, F.tot, sizeof(unsigned long long) * mfp_totals(F).words));
    AMC_HIP(c, st.get(meta, F.meta, sizeof meta));
    AMC_HIP(c, st.finish());
    bad = meta[0];
    if (meta[4]) return amc_fail(c, AMC_ERR_STATE, "%s", lost);
    if (bad != ~0ULL)
        return amc_fail(c, AMC_ERR_CAPACITY, "amc_mfp: a free path of particle %llu is outside [0, 2^-16 m) (or NaN); sampling stopped until amc_mfp_reset", bad);
    if (n_records) *n_records = (int64_t)meta[1];
    if (n_outside) *n_outside = (int64_t)meta[2];
    if (n_steps) *n_steps = F.n_steps;
    return AMC_OK;
}

int amc_mfp_load(amc_ctx *c, const int64_t *totals, const int64_t *hist, int64_t n_records, int64_t n_outside, int64_t n_steps)
{
    if (!c || !totals || n_records < 0 || n_outside < 0 || n_steps < 0) return AMC_ERR_INVALID;
    if (!c->MF.on) return amc_fail(c, AMC_ERR_STATE, "amc_mfp_load before amc_mfp_config");
    if (!hist && c->MF.g.hist_bins > 0) return amc_fail(c, AMC_ERR_INVALID, "amc_mfp_load: hist is NULL with hist_bins > 0");
    AMC_HIP(c, hipSetDevice(c->device));
    if (int rc = mfp_put(c, totals, hist, n_records, n_outside)) return rc;
    c->MF.n_steps = n_steps;
    return AMC_OK;
}

int amc_mfp_reset(amc_ctx *c)
{
    if (!c) return AMC_ERR_INVALID;
    if (int rc = amc_sampler_ready(c, c->MF.on, "amc_mfp", "reset")) return rc;
    if (int rc = mfp_put(c, nullptr, nullptr, 0, 0)) return rc;
    c->MF.n_steps = 0;
    return AMC_OK;
}

}  // extern "C"
