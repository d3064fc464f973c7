// amc_sample_dev.h — what the samplers share on the device, ONE copy of each piece: the bin rule of one axis (amc_fields_axis;
// amc_surface.hip through amc_surface_bin), a particle's frame (amc_sample_frame: its bin and its velocity components on the
// grid) and its bin alone (amc_sample_bin), the velocity quantisers' range, the carry-add into the 128-bit totals,
// the read of a particle's final state through the deferred results of the last sweep (amc_fields_lazy), and the shape of a
// streaming sampler's kernel pair: the walk over a workgroup's particles (amc_sample_walk, amc_sample_load_pair), its table's
// way into a slab row (amc_slab_begin, amc_slab_store) and the reduce of the slab into the running totals (k_slab_reduce).
// Every access goes through amc_g: global addresses.
#pragma once
#include "amc_internal.h"

#define AMC_SAMPLE_Q 7                  // integers per bin of a table in a slab row (fields: count, q1, q2; correlations: count, m, c; fluxes: two such tables)

// bin of one coordinate: -1 outside (below lo, at or beyond n bins, NaN); u == hi lands in the last bin
AMC_DEV int amc_fields_axis(double u, double lo, double hi, double w, int n)
{
    const double f = floor((u - lo) / w);
    if (!(f >= 0.0)) return -1;
    if (f >= (double)n) return (f == (double)n && u <= hi) ? n - 1 : -1;
    return (int)f;
}

// The frame of a particle on grid G: bin = its linear bin, -1 outside — (x, y, z) on a Cartesian grid, (r, z) on an axisymmetric
// one — and c = its velocity components there: (vx, vy, vz), or (radial, azimuthal, vz); on the axis itself (r == 0) vx, vy.
AMC_DEV bool amc_sample_frame(const amc_fields_grid_dev &G, double x, double y, double z, double vx, double vy, double vz, int &bin,
                              double (&c)[3])
{
    int i1, i2, i3;
    if (G.kind == AMC_FIELDS_CARTESIAN) {
        i1 = amc_fields_axis(x, G.lo[0], G.hi[0], G.w[0], G.n1);
        i2 = amc_fields_axis(y, G.lo[1], G.hi[1], G.w[1], G.n2);
        i3 = amc_fields_axis(z, G.lo[2], G.hi[2], G.w[2], G.n3);
        c[0] = vx; c[1] = vy; c[2] = vz;
    } else {
        const double r = sqrt(x * x + y * y);
        i1 = amc_fields_axis(r, G.lo[0], G.hi[0], G.w[0], G.n1);
        i2 = amc_fields_axis(z, G.lo[1], G.hi[1], G.w[1], G.n2);
        i3 = 0;
        if (r > 0.0) {
            c[0] = (x * vx + y * vy) / r;
            c[1] = (x * vy - y * vx) / r;
        } else {
            c[0] = vx; c[1] = vy;
        }
        c[2] = vz;
    }
    bin = -1;
    if (i1 < 0 || i2 < 0 || i3 < 0) return false;
    bin = (i1 * G.n2 + i2) * G.n3 + i3;
    return true;
}

// the linear bin of a position alone (the components fall away)
AMC_DEV int amc_sample_bin(const amc_fields_grid_dev &G, double x, double y, double z)
{
    int bin;
    double c[3];
    amc_sample_frame(G, x, y, z, 0.0, 0.0, 0.0, bin, c);
    return bin;
}

// the velocity quantisers' range: every component below 2^14 m/s in magnitude (false for NaN)
AMC_DEV bool amc_sample_speed_ok(double a, double b, double c) { return fabs(a) < 16384.0 && fabs(b) < 16384.0 && fabs(c) < 16384.0; }

// (lo, hi) += s: a partial sum that wrapped modulo 2^64 (its true value is below 2^63 in magnitude) into a signed 128-bit total
AMC_DEV void amc_add128(unsigned long long &lo, unsigned long long &hi, unsigned long long s)
{
    const unsigned long long now = lo + s;
    hi += (unsigned long long)(((long long)s < 0 ? -1LL : 0LL) + (now < lo ? 1LL : 0LL));
    lo = now;
}

// The state is read through the deferred results of the last sweep (amc_lazy: a particle that collided has its final state
// in the slot arrays until the next streaming pass picks it up) without consuming them: the step sequence is untouched.
// (A caller that does not look at the velocities passes dummies: their loads fall away.)
AMC_DEV void amc_fields_lazy(const amc_lazy &L, long long p, double &x, double &y, double &z, double &vx, double &vy, double &vz)
{
    if (L.enabled) {
        const int sl = amc_g(L.slot_of)[p];
        if (sl >= 0 && amc_g(L.moved)[sl]) {
            const auto *t = amc_g(L.state) + (size_t)sl * RS_SLOT_DOUBLES;
            x = t[0]; y = t[1]; z = t[2]; vx = t[3]; vy = t[4]; vz = t[5];
        }
    }
}

// ---- the streaming samplers' kernel pair: <sampler>_accum, one slab row per workgroup, and k_slab_reduce ----------------------------------
// The walk of an accumulate kernel: this workgroup's share [b0, b1) of the particles [lo, hi), as aligned pairs (2k, 2k + 1) — one
// 16-byte access per array and pair:
//     for (amc_sample_walk w(lo, hi); w.more(); w.next())       particle w.p0() is the workgroup's if w.v0(), w.p0() + 1 if w.v1()
// (one of them at the least: a share's odd ends are pairs of one).  A loop in the kernel, not a function that calls a lambda per
// pair: as a lambda the same body took 4 VGPRs more in k_moments_accum (68) and 2 in k_transit_accum (71).
struct amc_sample_walk {
    long long b0, b1, k;
    AMC_DEV amc_sample_walk(long long lo, long long hi)
    {
        const long long cnt = hi - lo;
        const long long per = (cnt + gridDim.x - 1) / gridDim.x;
        b0 = lo + per * blockIdx.x;
        b1 = b0 + per < hi ? b0 + per : hi;
        k = (b0 >> 1) + threadIdx.x;
        if (b0 >= b1) { b1 = 0; k = 0; }
    }
    AMC_DEV bool more() const { return 2 * k < b1; }
    AMC_DEV void next() { k += blockDim.x; }
    AMC_DEV long long p0() const { return 2 * k; }
    AMC_DEV bool v0() const { return 2 * k >= b0; }
    AMC_DEV bool v1() const { return 2 * k + 1 < b1; }
};

// Six values per particle out of the arrays A.x .. A.vz (amc_state, the correlations' origins) and back: a whole pair as six
// 16-byte accesses, one particle (element e) as six of 8 bytes.  amc_sample_load_pair chooses: element 0 if v0, element 1 if v1.
// (A kernel that loads from two sets of arrays puts both under ONE branch of its own, k_corr_accum: behind two calls of
// amc_sample_load_pair the second set's loads wait for the first's — measured + 2.0 us on the pore's 27.4 us lag sample.)
template <class A>
AMC_DEV void amc_sample_load_both(const A &S, long long p0, double (&x)[2], double (&y)[2], double (&z)[2], double (&vx)[2], double (&vy)[2],
                                  double (&vz)[2])
{
    const double2 ax = amc_g_load((const double2 *)(S.x + p0)), ay = amc_g_load((const double2 *)(S.y + p0));
    const double2 az = amc_g_load((const double2 *)(S.z + p0)), bx = amc_g_load((const double2 *)(S.vx + p0));
    const double2 by = amc_g_load((const double2 *)(S.vy + p0)), bz = amc_g_load((const double2 *)(S.vz + p0));
    x[0] = ax.x; x[1] = ax.y; y[0] = ay.x; y[1] = ay.y; z[0] = az.x; z[1] = az.y;
    vx[0] = bx.x; vx[1] = bx.y; vy[0] = by.x; vy[1] = by.y; vz[0] = bz.x; vz[1] = bz.y;
}
template <class A>
AMC_DEV void amc_sample_load_one(const A &S, long long p, int e, double (&x)[2], double (&y)[2], double (&z)[2], double (&vx)[2], double (&vy)[2],
                                 double (&vz)[2])
{
    x[e] = amc_g(S.x)[p]; y[e] = amc_g(S.y)[p]; z[e] = amc_g(S.z)[p];
    vx[e] = amc_g(S.vx)[p]; vy[e] = amc_g(S.vy)[p]; vz[e] = amc_g(S.vz)[p];
}
template <class A>
AMC_DEV void amc_sample_load_pair(const A &S, long long p0, bool v0, bool v1, double (&x)[2], double (&y)[2], double (&z)[2], double (&vx)[2],
                                  double (&vy)[2], double (&vz)[2])
{
    if (v0 && v1) amc_sample_load_both(S, p0, x, y, z, vx, vy, vz);
    else amc_sample_load_one(S, v0 ? p0 : p0 + 1, v0 ? 0 : 1, x, y, z, vx, vy, vz);
}
template <class A>
AMC_DEV void amc_sample_store_pair(const A &S, long long p0, bool v0, bool v1, const double (&x)[2], const double (&y)[2], const double (&z)[2],
                                   const double (&vx)[2], const double (&vy)[2], const double (&vz)[2])
{
    if (v0 && v1) {
        amc_g_store((double2 *)(S.x + p0), make_double2(x[0], x[1])); amc_g_store((double2 *)(S.y + p0), make_double2(y[0], y[1]));
        amc_g_store((double2 *)(S.z + p0), make_double2(z[0], z[1])); amc_g_store((double2 *)(S.vx + p0), make_double2(vx[0], vx[1]));
        amc_g_store((double2 *)(S.vy + p0), make_double2(vy[0], vy[1])); amc_g_store((double2 *)(S.vz + p0), make_double2(vz[0], vz[1]));
    } else {
        const long long p = v0 ? p0 : p0 + 1;
        const int e = v0 ? 0 : 1;
        amc_g(S.x)[p] = x[e]; amc_g(S.y)[p] = y[e]; amc_g(S.z)[p] = z[e];
        amc_g(S.vx)[p] = vx[e]; amc_g(S.vy)[p] = vy[e]; amc_g(S.vz)[p] = vz[e];
    }
}

// A workgroup's table of M words in LDS, zero before the walk (with its count of the particles outside, if it keeps one) ...
template <class Word>
AMC_DEV void amc_slab_begin(Word *tab, int M, unsigned int *outside_sum = nullptr)
{
    for (int j = threadIdx.x; j < M; j += blockDim.x) tab[j] = 0;
    if (outside_sum && threadIdx.x == 0) *outside_sum = 0;
    __syncthreads();
}
// ... and after it the workgroup's row of the slab, plain stores: [M][outside], or [M] alone
template <class Word>
AMC_DEV void amc_slab_store(Word *slab, const Word *tab, int M, const unsigned int *outside_sum = nullptr)
{
    __syncthreads();
    auto *row = amc_g(slab) + (size_t)blockIdx.x * (size_t)(M + (outside_sum ? 1 : 0));
    for (int j = threadIdx.x; j < M; j += blockDim.x) row[j] = tab[j];
    if (outside_sum && threadIdx.x == 0) row[M] = *outside_sum;
}

// The reduce: column j of the slab summed over its rows, for the sampler's Sink to add into its running totals.  64 columns per
// workgroup ((W + 1 + 63) / 64 of them), its sixteen waves take every sixteenth row, four loads in flight each: the rows are a
// chain of memory round trips otherwise (measured: 10 us for 123 rows with four waves).  A sum wraps modulo 2^64.  Sink, by value:
//   stopped()      the sampler has stopped: the launch adds nothing (the read reports why)
//   stride(W)      words per slab row: W + 1 where a row ends with the particles outside, else W
//   column(j, s)   the thread of totals column j < W, s its sum
//   counters(s)    the thread of j == W: the sample is counted; s is the sum of the outside column (0 where there is none)
//   companion      false — or true (the transits): a column may have a mate, the column beside it, whose sum goes into the same
//                  total.  mate(j): +1, the thread of column j sums column j + 1 too, and column(j, s, mate_sum) gets that sum as
//                  mate_sum(); -1, column j is such a mate and its own thread does nothing (two threads must not add into one
//                  total); 0, neither
#define AMC_SLAB_REDUCE_THREADS 1024
template <class Word, class Sink>
__global__ __launch_bounds__(AMC_SLAB_REDUCE_THREADS) void k_slab_reduce(const Word *slab, int rows, int W, Sink sink)
{
    if (sink.stopped()) return;
    constexpr int WAVES = AMC_SLAB_REDUCE_THREADS / 64;
    __shared__ unsigned long long part[Sink::companion ? 2 : 1][WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + lane;
    const size_t stride = (size_t)sink.stride(W);
    int mate = 0;
    if constexpr (Sink::companion) mate = sink.mate(j);
    unsigned long long s = 0, s1 = 0;
    if ((size_t)j < stride) {
        const auto *col = amc_g(slab) + j;
#pragma unroll 4
        for (int b = wave; b < rows; b += WAVES) {
            s += col[(size_t)b * stride];
            if constexpr (Sink::companion) if (mate > 0) s1 += col[(size_t)b * stride + 1];
        }
    }
    part[0][wave][lane] = s;
    if constexpr (Sink::companion) part[1][wave][lane] = s1;
    __syncthreads();
    if (wave != 0 || j > W || mate < 0) return;
    auto total = [&](int t) {
        unsigned long long a = 0;
#pragma unroll
        for (int k = 0; k < WAVES; k++) a += part[t][k][lane];
        return a;
    };
    if (j == W) sink.counters(total(0));
    else if constexpr (Sink::companion) sink.column(j, total(0), [&] { return total(1); });
    else sink.column(j, total(0));
}
template <class Word, class Sink>
static hipError_t amc_launch_slab_reduce(amc_ctx *c, const Word *slab, int rows, int W, Sink sink)
{
    amc_prof_begin(c, AMC_K_FIELDS);
    AMC_LAUNCH(c, (k_slab_reduce<Word, Sink>), dim3((W + 1 + 63) / 64), dim3(AMC_SLAB_REDUCE_THREADS), slab, rows, W, sink);
    amc_prof_end(c);
    return hipGetLastError();
}
