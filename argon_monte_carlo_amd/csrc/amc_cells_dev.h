// amc_cells_dev.h — what the whole-system neighbour searches over counting-sort cells share on the device, ONE copy of each piece
// (the pair sampler, amc_pair.hip, and the overlap removal of a synthetic start, amc_ic.hip): the exclusive scan of the cells'
// counts into the cells' offsets, its launch geometry, and the broadcast of one lane's double.  Every access goes through amc_g.
#pragma once
#include <algorithm>

#include "amc_internal.h"
#include "amc_device.h"

AMC_DEV double pair_lane(double v, int k)   // lane k's value of v, k uniform
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), k), __builtin_amdgcn_readlane(__double2loint(v), k));
}

// cell_off = exclusive scan of cell_count, cell_off[ncells] = the records; cell_count = 0 for the next search.  Two launches of
// the same geometry (pair_scan_geometry workgroups): every WAVE of the grid has a contiguous segment of `seg` cells (a multiple of
// 64) and walks it 64 cells at a time, lane by lane — coalesced reads and writes.  k_pair_scan_sums leaves the segments' sums in
// wave_sum; k_pair_scan adds up the sums of the waves before its own (at most AMC_PAIR_SCAN_MAX_BLOCKS * 16 of them, read across
// the lanes) and walks its segment again for the offsets: a scan of 64 values across the lanes and a running carry.
// (static: every translation unit that includes the header launches its own instance.)
#define AMC_PAIR_SCAN_THREADS 1024
#define AMC_PAIR_SCAN_WAVES (AMC_PAIR_SCAN_THREADS / 64)
#define AMC_PAIR_SCAN_MAX_BLOCKS 128
#define AMC_PAIR_SCAN_CELLS_PER_BLOCK 16384     // 1,024 cells per wave: sixteen passes of 64
AMC_DEV unsigned int pair_wave_sum(unsigned int s)
{
    for (int d = 32; d; d >>= 1) s += __shfl_xor(s, d);
    return s;
}

static __global__ __launch_bounds__(AMC_PAIR_SCAN_THREADS) void k_pair_scan_sums(const unsigned int *cell_count, unsigned int *wave_sum, int ncells, int seg)
{
    const int lane = threadIdx.x & 63, wave = blockIdx.x * AMC_PAIR_SCAN_WAVES + (threadIdx.x >> 6);
    const long long a0 = (long long)wave * seg;
    const int a = (int)(a0 < ncells ? a0 : ncells), b = min(a + seg, ncells);
    const auto *cnt = amc_g(cell_count);
    unsigned int s = 0;
    for (int c = a + lane; c < b; c += 64) s += cnt[c];
    s = pair_wave_sum(s);
    if (lane == 0) amc_g(wave_sum)[wave] = s;
}

static __global__ __launch_bounds__(AMC_PAIR_SCAN_THREADS) void k_pair_scan(unsigned int *cell_count, unsigned int *cell_off, const unsigned int *wave_sum,
                                                                            int ncells, int seg)
{
    const int lane = threadIdx.x & 63, wave = blockIdx.x * AMC_PAIR_SCAN_WAVES + (threadIdx.x >> 6);
    const int nwaves = gridDim.x * AMC_PAIR_SCAN_WAVES;
    const long long a0 = (long long)wave * seg;
    const int a = (int)(a0 < ncells ? a0 : ncells), b = min(a + seg, ncells);
    auto *cnt = amc_g(cell_count);
    auto *off = amc_g(cell_off);
    unsigned int before = 0;
    for (int k = lane; k < wave; k += 64) before += amc_g(wave_sum)[k];
    unsigned int run = pair_wave_sum(before);
    for (int t = a; t < b; t += 64) {
        const int c = t + lane;
        const unsigned int v = c < b ? cnt[c] : 0u;
        unsigned int inc = v;           // inclusive scan across the lanes
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned int u = __shfl_up(inc, d);
            if (lane >= d) inc += u;
        }
        if (c < b) { off[c] = run + (inc - v); cnt[c] = 0; }
        run += __shfl(inc, 63);
    }
    if (wave == nwaves - 1 && lane == 63) off[ncells] = run;       // (the last wave: everything before it and its own segment)
}

// workgroups of the scan's two launches and the cells per wave
static void pair_scan_geometry(int ncells, int *blocks, int *seg)
{
    *blocks = std::max(1, std::min(AMC_PAIR_SCAN_MAX_BLOCKS, (ncells + AMC_PAIR_SCAN_CELLS_PER_BLOCK - 1) / AMC_PAIR_SCAN_CELLS_PER_BLOCK));
    const int waves = *blocks * AMC_PAIR_SCAN_WAVES;
    *seg = (ncells + waves * 64 - 1) / (waves * 64) * 64;
}
