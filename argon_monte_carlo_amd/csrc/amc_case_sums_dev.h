// amc_case_sums_dev.h — the sums of one device-RNG step (z-momentum, energy to the cold walls, energy to the hot walls) from
// the per-hit records of the seven energised cases.  fp64 addition depends on its order, and the order is stated here and
// nowhere else: per case the hits in ASCENDING PARTICLE INDEX, failed contact solves skipped, m_case = m_case + dpz and
// e_case = e_case + dE left to right from 0.0 (k_case_sums, and amc_temp_device_sums on the host's copies); then the cases
// folded in the order 3..9 (amc_fold_cases, called by both).
#pragma once
#include "amc_internal.h"

// a record count as the kernels use it: nothing below 0 and nothing beyond the segment's capacity is read
template <class T>
__host__ __device__ inline int amc_clamp_count(T cnt, int cap) { return cnt < 0 ? 0 : (cnt < cap ? (int)cnt : cap); }

__host__ __device__ inline bool amc_case_cold(int case_id) { return case_id == 3 || case_id == 7 || case_id == 9; }
__host__ __device__ inline bool amc_case_hot(int case_id) { return case_id == 4 || case_id == 6 || case_id == 8; }

// The fold of the cases, slot s = case 3 + s: m[s] and e[s] are the case's ordered sums, any[s] says that a record with a
// good contact solve went into them, present[s] that the case had records at all (a case without records adds nothing; one
// whose every solve failed adds its 0.0 and sets no bit).  The gap case (5) adds momentum only.
__host__ __device__ inline amc_temp_row amc_fold_cases(const double *m, const double *e, const int *any, const int *present)
{
    amc_temp_row r;
    r.sums[0] = r.sums[1] = r.sums[2] = 0.0; r.had = 0; r.pad = 0;
    for (int s = 0; s < 7; s++) {
        if (!present[s]) continue;
        r.sums[0] = r.sums[0] + m[s];
        if (any[s]) r.had |= 1u;
        if (amc_case_cold(3 + s)) { r.sums[1] = r.sums[1] + e[s]; if (any[s]) r.had |= 2u; }
        if (amc_case_hot(3 + s)) { r.sums[2] = r.sums[2] + e[s]; if (any[s]) r.had |= 4u; }
    }
    return r;
}

// the segment q with off[q] <= i < off[q + 1] (i below off[nseg]; empty segments are passed over)
__device__ inline int case_sums_segment(const int *off, int nseg, int i)
{
    int lo = 0, hi = nseg - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (i >= off[mid + 1]) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// k_case_sums: ONE workgroup forms the step's sums and writes them as row `row_index` of the series.  The records come in
// 7 * world segments, each in the order its atomics happened to run: segment q = s * world + r holds the hits of case 3 + s
// with the particle indices of range r, the ranges ascending with r.  A particle hits a case at most once per step, so the
// RANK of a record — the records of its segment with a smaller particle index — is its place inside the segment, and the
// segments of a case in the order of r are the case's hits in ascending particle index.  Counting ranks is quadratic in a
// segment's records but needs no exchange between threads.  Lanes 0..6 then add one case each, lane 0 folds the cases.
//
// `Source` says where the records are and is all that differs between the uses (amc_energised.hip: one context's seven
// segments; amc_hits.hip: the blocks of all ranks):
//   MAX_WORLD        the largest world it is launched with (sizes the offset table)
//   nseg()           7 * world
//   count(q), cap()  the raw count of segment q (clamped here) and the capacity of every segment
//   segment(q)       a view with key(k) — the particle index —, ok(k), dpz(k) and dE(k) of its record k
// A step of at most `tile` (<= TILE) records is ordered in LDS; a larger one takes the same steps through `perm`
// ([nseg * cap]) in global memory: slow, and as exact.  A count above the capacity: (case, row, count) into ovf[0..2] once
// — the run then fails with AMC_ERR_CAPACITY and hands out none of its rows — and no row is written from truncated data.
template <class Source, int THREADS, int TILE>
__global__ __launch_bounds__(THREADS) void k_case_sums(Source src, int *__restrict__ perm, amc_temp_row *__restrict__ row, int row_index,
                                                       int *__restrict__ ovf, int tile)
{
    constexpr int PER_THREAD = TILE / THREADS, MAX_SEG = 7 * Source::MAX_WORLD;     // records of the LDS path a thread handles
    static_assert(TILE % THREADS == 0, "the tile is a multiple of the workgroup");
    __shared__ int s_key[TILE];
    __shared__ double s_dpz[TILE], s_dE[TILE];
    __shared__ unsigned char s_ok[TILE];
    __shared__ int s_off[MAX_SEG + 1];
    __shared__ double s_m[7], s_e[7];
    __shared__ int s_any[7], s_lost;
    __shared__ long long s_cnt[MAX_SEG];
    const int tid = threadIdx.x, nseg = src.nseg(), world = nseg / 7, cap = src.cap();
    for (int q = tid; q < nseg; q += THREADS) s_cnt[q] = src.count(q);       // (the counts side by side: one round trip, not nseg)
    __syncthreads();
    if (tid == 0) {
        int off = 0, lost = 0;
        for (int q = 0; q < nseg; q++) {
            const long long cnt = s_cnt[q];
            if (cnt > cap) {
                if (ovf[0] == 0) { ovf[1] = row_index; ovf[2] = (int)cnt; ovf[0] = 3 + q / world; }
                lost = 1;
            }
            s_off[q] = off;
            off += amc_clamp_count(cnt, cap);
        }
        s_off[nseg] = off;
        s_lost = lost;
    }
    __syncthreads();
    if (s_lost) return;
    const int total = s_off[nseg];
    const bool tiled = total <= tile;
    if (tiled) {
        // a thread's (at most PER_THREAD) records: segment by binary search, all four fields loaded side by side
        int seg_of[PER_THREAD], key[PER_THREAD];
        double dpz[PER_THREAD], dE[PER_THREAD];
        bool ok[PER_THREAD];
#pragma unroll
        for (int it = 0; it < PER_THREAD; it++) {
            const int i = tid + it * THREADS;
            seg_of[it] = 0; key[it] = 0; dpz[it] = 0.0; dE[it] = 0.0; ok[it] = false;
            if (i >= total) continue;
            const int q = case_sums_segment(s_off, nseg, i), k = i - s_off[q];
            const auto R = src.segment(q);
            seg_of[it] = q; key[it] = R.key(k); ok[it] = R.ok(k); dpz[it] = R.dpz(k); dE[it] = R.dE(k);
        }
#pragma unroll
        for (int it = 0; it < PER_THREAD; it++) {
            const int i = tid + it * THREADS;
            if (i < total) s_key[i] = key[it];
        }
        __syncthreads();
#pragma unroll
        for (int it = 0; it < PER_THREAD; it++) {
            const int i = tid + it * THREADS;
            if (i >= total) continue;
            const int q = seg_of[it], n = s_off[q + 1] - s_off[q];
            const int mine = key[it];
            const int *v = s_key + s_off[q];
            int rank = 0, j = 0;
            for (; j + 8 <= n; j += 8) {            // (loads side by side, as in the additions below)
                int t[8];
#pragma unroll
                for (int e = 0; e < 8; e++) t[e] = v[j + e];
#pragma unroll
                for (int e = 0; e < 8; e++) rank += t[e] < mine ? 1 : 0;
            }
            for (; j < n; j++) rank += v[j] < mine ? 1 : 0;
            const int at = s_off[q] + rank;
            s_dpz[at] = dpz[it]; s_dE[at] = dE[it]; s_ok[at] = ok[it] ? 1 : 0;
        }
    } else {
        for (int i = tid; i < total; i += THREADS) {
            const int q = case_sums_segment(s_off, nseg, i);
            const auto R = src.segment(q);
            const int k = i - s_off[q], n = s_off[q + 1] - s_off[q];
            const int mine = R.key(k);
            int rank = 0;
            for (int j = 0; j < n; j++) rank += R.key(j) < mine ? 1 : 0;
            perm[(size_t)q * (size_t)cap + rank] = k;
        }
    }
    __syncthreads();
    if (tid < 7) {
        const int s = tid;
        double m_case = 0.0, e_case = 0.0;
        int any = 0;
        if (tiled) {
            // the case's records stand in LDS in the order they are added: segment by segment, place by place.  Sixteen at a
            // time: the loads side by side, then the additions in order (a lane's chain is the latency of its loads otherwise:
            // over 8 ranks at N = 4e6, where case 9 has 1,900 hits, the kernel took 327 us when each record was loaded, tested
            // and added in turn).  The additions stay `if` statements: behind a function that takes the sums by reference
            // the compiler waits for all seventeen loads before the first addition, which cost 4 % of the kernel.
            const int end = s_off[(s + 1) * world];
            int u = s_off[s * world];
            for (; u + 16 <= end; u += 16) {
                double a[16], b[16];
                unsigned char ok[16];
#pragma unroll
                for (int j = 0; j < 16; j++) { a[j] = s_dpz[u + j]; b[j] = s_dE[u + j]; ok[j] = s_ok[u + j]; }
#pragma unroll
                for (int j = 0; j < 16; j++)
                    if (ok[j]) { m_case = m_case + a[j]; e_case = e_case + b[j]; any = 1; }
            }
            for (; u < end; u++)
                if (s_ok[u]) { m_case = m_case + s_dpz[u]; e_case = e_case + s_dE[u]; any = 1; }
        } else {
            for (int q = s * world; q < (s + 1) * world; q++) {
                const int n = s_off[q + 1] - s_off[q];
                const auto R = src.segment(q);
                for (int u = 0; u < n; u++) {
                    const int k = perm[(size_t)q * (size_t)cap + u];
                    const bool ok = R.ok(k);
                    const double a = R.dpz(k), b = R.dE(k);         // (beside ok's load, not behind it)
                    if (ok) { m_case = m_case + a; e_case = e_case + b; any = 1; }
                }
            }
        }
        s_m[s] = m_case; s_e[s] = e_case; s_any[s] = any;
    }
    __syncthreads();
    if (tid == 0) {
        int present[7];
#pragma unroll
        for (int s = 0; s < 7; s++) present[s] = s_off[(s + 1) * world] != s_off[s * world];
        row[row_index] = amc_fold_cases(s_m, s_e, s_any, present);
    }
}
