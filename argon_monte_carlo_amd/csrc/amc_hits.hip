// amc_hits.hip — the third collective of a sharded device-RNG step: the per-hit results of the seven
// energised cases travel in one small block per rank, and every rank forms the step's sums from the blocks of all ranks
// exactly as a single context's k_temp_sums (amc_energised.hip) forms them from its own segments.
//
// One block, in 8-byte words (the same on every rank: Hc depends on the whole system's n only):
//   [0..6]  hits of case 3 + s as the owner counted them (AMC_HITS_LOST when they exceeded its record segment), [7] unused
//   then per case s three arrays of Hc words: key = particle | ok << 32, dp_z, dE        (8 + 21 Hc words)
// Shards are ascending index ranges and the blocks stand in rank order, so the place of a record among its case's hits in
// ascending particle index is: the hits of that case in the lower ranks' blocks + its rank inside its own block.
#include <algorithm>

#include "amc_internal.h"

#define AMC_HITS_HEADER 8
#define AMC_HITS_LOST 0x7fffffffLL
#define AMC_HITS_TILE 6144          // records a step may have for the LDS path: 21 B each, 126 KiB of the CU's 160 (a step at N = 4e6 has about 2,500)
#define AMC_HITS_THREADS 1024
#define AMC_HITS_PER_THREAD (AMC_HITS_TILE / AMC_HITS_THREADS)    // records of the LDS path a thread handles (the tile is a multiple)

// the segment q with off[q] <= i < off[q + 1] (i below off[nseg]; empty segments are passed over)
__device__ inline int hits_segment(const int *off, int nseg, int i)
{
    int lo = 0, hi = nseg - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (i >= off[mid + 1]) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// k_hits_pack: grid (ceil(Hc / 256), 7) — the rank's seven segments into its send block.  Counts are clamped to the segment
// capacity as k_temp_sums clamps them; a count above Hc is flagged (ovf[3]) and travels as it is, so every receiver sees it.
__global__ __launch_bounds__(256) void k_hits_pack(temp_dev_segments D, long long *__restrict__ blk, int Hc, int *__restrict__ ovf)
{
    const int s = blockIdx.y, k = blockIdx.x * blockDim.x + threadIdx.x;
    const int cnt = D.count[s];
    const int n = cnt < 0 ? 0 : (cnt < D.cap ? cnt : D.cap);
    if (k == 0) {
        blk[s] = cnt > D.cap ? AMC_HITS_LOST : (long long)n;
        if (s == 0) blk[7] = 0;
        if (cnt > D.cap || n > Hc) ovf[3] = 1;
    }
    if (k >= n || k >= Hc) return;
    const size_t seg = (size_t)s * (size_t)D.cap + (size_t)k;
    long long *rec = blk + AMC_HITS_HEADER + (size_t)3 * (size_t)s * (size_t)Hc;
    rec[k] = (long long)(unsigned int)D.idx[seg] | ((long long)(D.ok[seg] ? 1 : 0) << 32);
    ((double *)rec)[(size_t)Hc + k] = D.dpz[seg];
    ((double *)rec)[2 * (size_t)Hc + k] = D.dE[seg];
}

// k_hits_sums: ONE workgroup over the blocks of all ranks.  k_temp_sums's additions one for one: per case m_case = m_case +
// dpz and e_case = e_case + dE left to right from 0.0 in ascending particle index over all ranks, records with ok == 0
// skipped, then the cases folded in order 3..9 into row `row_index` of the series.  Segment q = s * world + r holds the hits
// of case 3 + s that rank r owns.  A step whose records exceed the LDS tile orders them through `perm` in global memory
// (slow, and as exact; AMC_MG_HITS_TILE=k lowers the tile so that a test reaches that path with a few hundred hits).
// A block over capacity: (case, row, count) into ovf[0..2] — the same words on every rank, which all read the same blocks —
// and no row is written.
__global__ __launch_bounds__(AMC_HITS_THREADS) void k_hits_sums(const long long *__restrict__ recv, int world, long long blk_words, int Hc,
                                                                 int *__restrict__ perm, amc_temp_row *__restrict__ row, int row_index,
                                                                 int *__restrict__ ovf, int tile)
{
    __shared__ int s_key[AMC_HITS_TILE];
    __shared__ double s_dpz[AMC_HITS_TILE], s_dE[AMC_HITS_TILE];
    __shared__ unsigned char s_ok[AMC_HITS_TILE];
    __shared__ int s_off[7 * AMC_MG_HITS_MAX_WORLD + 1];
    __shared__ double s_m[7], s_e[7];
    __shared__ int s_any[7], s_lost;
    __shared__ long long s_cnt[7 * AMC_MG_HITS_MAX_WORLD];
    const int tid = threadIdx.x, nseg = 7 * world;
    for (int q = tid; q < nseg; q += AMC_HITS_THREADS) {         // (the headers side by side: one round trip, not 7 x world)
        const int s = q / world, r = q - s * world;
        s_cnt[q] = recv[(size_t)r * (size_t)blk_words + s];
    }
    __syncthreads();
    if (tid == 0) {
        int off = 0, lost = 0;
        for (int q = 0; q < nseg; q++) {
            const int s = q / world;
            const long long cnt = s_cnt[q];
            if (cnt > Hc) {
                if (ovf[0] == 0) { ovf[1] = row_index; ovf[2] = (int)cnt; ovf[0] = 3 + s; }
                lost = 1;
            }
            s_off[q] = off;
            off += cnt < 0 ? 0 : (cnt < Hc ? (int)cnt : Hc);
        }
        s_off[nseg] = off;
        s_lost = lost;
    }
    __syncthreads();
    if (s_lost) return;                 // (the run fails with AMC_ERR_CAPACITY: no row from truncated data)
    const int total = s_off[nseg];
    const bool tiled = total <= tile;          // (tile <= AMC_HITS_TILE: the launcher)
    if (tiled) {
        // a thread's (at most AMC_HITS_PER_THREAD) records: segment by binary search, all four fields loaded side by side
        int seg_of[AMC_HITS_PER_THREAD];
        long long key[AMC_HITS_PER_THREAD];
        double dpz[AMC_HITS_PER_THREAD], dE[AMC_HITS_PER_THREAD];
#pragma unroll
        for (int it = 0; it < AMC_HITS_PER_THREAD; it++) {
            const int i = tid + it * AMC_HITS_THREADS;
            seg_of[it] = 0; key[it] = 0; dpz[it] = 0.0; dE[it] = 0.0;
            if (i >= total) continue;
            const int q = hits_segment(s_off, nseg, i);
            const int s = q / world, r = q - s * world, k = i - s_off[q];
            const long long *rec = recv + (size_t)r * (size_t)blk_words + AMC_HITS_HEADER + (size_t)3 * (size_t)s * (size_t)Hc;
            seg_of[it] = q; key[it] = rec[k];
            dpz[it] = ((const double *)rec)[(size_t)Hc + k]; dE[it] = ((const double *)rec)[2 * (size_t)Hc + k];
        }
#pragma unroll
        for (int it = 0; it < AMC_HITS_PER_THREAD; it++) {
            const int i = tid + it * AMC_HITS_THREADS;
            if (i < total) s_key[i] = (int)(unsigned int)key[it];
        }
        __syncthreads();
#pragma unroll
        for (int it = 0; it < AMC_HITS_PER_THREAD; it++) {
            const int i = tid + it * AMC_HITS_THREADS;
            if (i >= total) continue;
            const int q = seg_of[it], n = s_off[q + 1] - s_off[q];
            const int mine = (int)(unsigned int)key[it];
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
            s_dpz[at] = dpz[it]; s_dE[at] = dE[it]; s_ok[at] = (unsigned char)((key[it] >> 32) & 1);
        }
    } else {
        for (int i = tid; i < total; i += AMC_HITS_THREADS) {
            const int q = hits_segment(s_off, nseg, i);
            const int s = q / world, r = q - s * world;
            const long long *rec = recv + (size_t)r * (size_t)blk_words + AMC_HITS_HEADER + (size_t)3 * (size_t)s * (size_t)Hc;
            const int k = i - s_off[q], n = s_off[q + 1] - s_off[q];
            const int mine = (int)(unsigned int)rec[k];
            int rank = 0;
            for (int j = 0; j < n; j++) rank += (int)(unsigned int)rec[j] < mine ? 1 : 0;
            perm[(size_t)q * (size_t)Hc + rank] = k;
        }
    }
    __syncthreads();
    if (tid < 7) {
        const int s = tid;
        double m_case = 0.0, e_case = 0.0;
        int any = 0;
        if (tiled) {
            // the case's records stand in LDS in the order they are added: rank by rank, place by place.  Sixteen at a time: the
            // loads side by side, then the additions in order (a lane's chain is the latency of its loads otherwise: the
            // kernel took 327 us at N = 4e6, where case 9 has 1,900 hits, when each record was loaded, tested and added in turn)
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
            for (int r = 0; r < world; r++) {
                const int q = s * world + r, n = s_off[q + 1] - s_off[q];
                const long long *rec = recv + (size_t)r * (size_t)blk_words + AMC_HITS_HEADER + (size_t)3 * (size_t)s * (size_t)Hc;
                for (int u = 0; u < n; u++) {
                    const int k = perm[(size_t)q * (size_t)Hc + u];
                    if (!((rec[k] >> 32) & 1)) continue;
                    m_case = m_case + ((const double *)rec)[(size_t)Hc + k];
                    e_case = e_case + ((const double *)rec)[2 * (size_t)Hc + k];
                    any = 1;
                }
            }
        }
        s_m[s] = m_case; s_e[s] = e_case; s_any[s] = any;
    }
    __syncthreads();
    if (tid == 0) {
        double sums[3] = {0.0, 0.0, 0.0};
        unsigned int had = 0;
        for (int s = 0; s < 7; s++) {
            if (s_off[(s + 1) * world] == s_off[s * world]) continue;
            const int case_id = 3 + s;
            sums[0] = sums[0] + s_m[s];
            if (s_any[s]) had |= 1u;
            const bool cold = (case_id == 3 || case_id == 7 || case_id == 9), hot = (case_id == 4 || case_id == 6 || case_id == 8);
            if (cold) { sums[1] = sums[1] + s_e[s]; if (s_any[s]) had |= 2u; }
            if (hot) { sums[2] = sums[2] + s_e[s]; if (s_any[s]) had |= 4u; }
        }
        amc_temp_row r;
        r.sums[0] = sums[0]; r.sums[1] = sums[1]; r.sums[2] = sums[2]; r.had = had; r.pad = 0;
        row[row_index] = r;
    }
}

int64_t amc_hits_block_words(int hits_cap) { return AMC_HITS_HEADER + 21 * (int64_t)hits_cap; }

hipError_t amc_launch_hits_pack(amc_ctx *c)
{
    const amc_mg_ws &M = c->MG;
    amc_prof_begin(c, AMC_K_BIN_SCAN);          // (a class no other kernel uses: the rehearsal reads the two kernels separately)
    AMC_LAUNCH(c, k_hits_pack, dim3((unsigned)((M.hits_cap + 255) / 256), 7), dim3(256), c->TD.seg, M.hits_send, M.hits_cap, c->TD.ovf);
    amc_prof_end(c);
    return hipGetLastError();
}

hipError_t amc_launch_hits_sums(amc_ctx *c, int world, int64_t row)
{
    const amc_mg_ws &M = c->MG;
    amc_prof_begin(c, AMC_K_BIN_SCATTER);
    AMC_LAUNCH(c, k_hits_sums, dim3(1), dim3(AMC_HITS_THREADS), (const long long *)M.hits_recv, world,
               (long long)amc_hits_block_words(M.hits_cap), M.hits_cap, M.hits_perm, c->TD.series, (int)row, c->TD.ovf,
               std::min(std::max(M.hits_tile, 0), AMC_HITS_TILE));
    amc_prof_end(c);
    return hipGetLastError();
}
