// amc_hits.hip — the third collective of a sharded device-RNG step: the per-hit results of the seven
// energised cases travel in one small block per rank, and every rank forms the step's sums from the blocks of all ranks with
// the kernel a single context forms them with from its own segments (k_case_sums, amc_case_sums_dev.h).
//
// One block, in 8-byte words (the same on every rank: Hc depends on the whole system's n only):
//   [0..6]  hits of case 3 + s as the owner counted them (AMC_HITS_LOST when they exceeded its record segment), [7] unused
//   then per case s three arrays of Hc words: key = particle | ok << 32, dp_z, dE        (8 + 21 Hc words)
// Shards are ascending index ranges and the blocks stand in rank order, so the place of a record among its case's hits in
// ascending particle index is: the hits of that case in the lower ranks' blocks + its rank inside its own block.
#include <algorithm>

#include "amc_case_sums_dev.h"

#define AMC_HITS_HEADER 8
#define AMC_HITS_LOST 0x7fffffffLL
#define AMC_HITS_TILE 6144          // records a step may have for the LDS path: 21 B each, 126 KiB of the CU's 160 (a step at N = 4e6 has about 2,500)
#define AMC_HITS_THREADS 1024

// k_hits_pack: grid (ceil(Hc / 256), 7) — the rank's seven segments into its send block.  Counts are clamped to the segment
// capacity; a count above Hc is flagged (ovf[3]) and travels as it is, so every receiver sees it.
__global__ __launch_bounds__(256) void k_hits_pack(temp_dev_segments D, long long *__restrict__ blk, int Hc, int *__restrict__ ovf)
{
    const int s = blockIdx.y, k = blockIdx.x * blockDim.x + threadIdx.x;
    const int cnt = D.count[s];
    const int n = amc_clamp_count(cnt, D.cap);
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

// The blocks of all ranks as k_case_sums's source: segment q = s * world + r is case 3 + s in the block of rank r.  A count
// above Hc (AMC_HITS_LOST included) fails the run with the same words on every rank, which all read the same blocks.
// (AMC_MG_HITS_TILE=k lowers the tile so that a test reaches the path through global memory with a few hundred hits.)
struct hits_blocks {
    static constexpr int MAX_WORLD = AMC_MG_HITS_MAX_WORLD;
    const long long *recv;
    long long blk_words;
    int world, Hc;
    struct view {
        const long long *rec;
        int Hc;
        __device__ int key(int k) const { return (int)(unsigned int)rec[k]; }
        __device__ bool ok(int k) const { return (rec[k] >> 32) & 1; }
        __device__ double dpz(int k) const { return ((const double *)rec)[(size_t)Hc + k]; }
        __device__ double dE(int k) const { return ((const double *)rec)[2 * (size_t)Hc + k]; }
    };
    __device__ int nseg() const { return 7 * world; }
    __device__ int cap() const { return Hc; }
    __device__ long long count(int q) const { return recv[(size_t)(q % world) * (size_t)blk_words + q / world]; }
    __device__ view segment(int q) const
    {
        const int s = q / world, r = q - s * world;
        return view{recv + (size_t)r * (size_t)blk_words + AMC_HITS_HEADER + (size_t)3 * (size_t)s * (size_t)Hc, Hc};
    }
};

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
    const hits_blocks src = {(const long long *)M.hits_recv, (long long)amc_hits_block_words(M.hits_cap), world, M.hits_cap};
    amc_prof_begin(c, AMC_K_BIN_SCATTER);
    AMC_LAUNCH(c, (k_case_sums<hits_blocks, AMC_HITS_THREADS, AMC_HITS_TILE>), dim3(1), dim3(AMC_HITS_THREADS), src, M.hits_perm,
               c->TD.series, (int)row, c->TD.ovf, std::min(std::max(M.hits_tile, 0), AMC_HITS_TILE));
    amc_prof_end(c);
    return hipGetLastError();
}
