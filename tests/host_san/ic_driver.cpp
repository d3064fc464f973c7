// ic_driver.cpp — drives amc_init_separate's host code (include/argonmc-ic.h) over the stand-in HIP runtime (hip_shim.cpp) under
// AddressSanitizer and UBSan: what the call refuses, the smallest systems, the launches of one search, and an allocation failure
// at every allocation of the call.  Kernels do not run here: the counts the call reads back are what its own memset left, zero,
// so a search finds nothing and the loop ends after it.  Plain C++ against include/argonmc.h; exits non-zero on a wrong return
// code, a wrong count or an object left behind.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <vector>

#include "argonmc.h"
#include "hip_shim.h"

#define FAIL(...)                                                  \
    do {                                                           \
        fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__);       \
        fprintf(stderr, __VA_ARGS__);                              \
        fputc('\n', stderr);                                       \
        fflush(stdout);                                            \
        fflush(stderr);                                            \
        _exit(1);                                                  \
    } while (0)
#define EXPECT(c, call, want)                                                                                          \
    do {                                                                                                               \
        const int rc_ = (call);                                                                                        \
        if (rc_ != (want)) FAIL("%s returned %d, expected %d: %s", #call, rc_, (int)(want), amc_last_error(c));        \
    } while (0)
#define OK(c, call) EXPECT(c, call, AMC_OK)
#define CHECK(cond, ...) do { if (!(cond)) FAIL(__VA_ARGS__); } while (0)

static amc_params cube_params(int64_t n)
{
    amc_params p;
    memset(&p, 0, sizeof p);
    const double ar = sqrt(3.6e-19 / (4.0 * M_PI));
    p.struct_size = (int32_t)sizeof p;
    p.geometry = AMC_GEOM_CUBE;
    p.n = n;
    p.collision_range = 2.0 * ar;
    p.argon_mass = 6.63e-26;
    p.argon_radius = ar;
    p.hist_bins = 200;
    p.hist_lo = 0.0;
    p.hist_hi = 1e-6;
    p.max_paths = 64;
    p.nx = p.ny = p.nz = 15;
    p.cube_x = p.cube_y = p.cube_z = 100e-9;
    p.dx = p.dy = p.dz = 100e-9 / 15;
    p.overlap_x = p.overlap_y = p.overlap_z = p.dx / 10;
    return p;
}

static amc_ic_config cube_config(uint64_t seed)
{
    amc_ic_config g;
    memset(&g, 0, sizeof g);
    g.struct_size = (int32_t)sizeof g;
    g.seed = seed;
    g.a_shape = 300.0;
    return g;
}

static void upload(amc_ctx *c, int64_t n)
{
    std::vector<double> a((size_t)n);
    std::vector<uint8_t> f((size_t)n, 0);
    for (int64_t k = 0; k < n; k++) a[(size_t)k] = 100e-9 * (k + 0.5) / (double)n;
    OK(c, amc_upload(c, a.data(), a.data(), a.data(), a.data(), a.data(), a.data(), a.data(), a.data(), a.data(), a.data(), f.data()));
}

static int64_t owned(amc_ctx *c)
{
    int64_t k = -1;
    OK(c, amc_owned_count(c, &k));
    return k;
}

static void no_bad_launches(const char *where)
{
    const long bad = shim_bad_launch_count();
    for (long k = 0; k < bad && k < 20; k++) fprintf(stderr, "bad launch: %s\n", shim_bad_launch(k));
    if (bad) FAIL("%ld refused launch(es) in %s", bad, where);
}

static const int64_t POISON = 0x1111111111111111LL;

int main()
{
    const amc_ic_config cfg = cube_config(7);
    const double d = 3.4e-10;

    // ---- without a context, and what a context refuses: nothing allocated, nothing launched ------------------------------------------
    int64_t st[AMC_IC_STATS];
    CHECK(amc_init_separate(nullptr, &cfg, d, 1, 1, st) == AMC_ERR_INVALID, "a null context was not refused");
    amc_params p = cube_params(1000);
    amc_ctx *c = nullptr;
    OK(c, amc_create(&c, &p));
    EXPECT(c, amc_init_separate(c, nullptr, d, 1, 1, st), AMC_ERR_INVALID);
    const int64_t own0 = owned(c);
    const long launches0 = shim_launch_count();
    EXPECT(c, amc_init_separate(c, &cfg, d, 1, 1, st), AMC_ERR_STATE);          // no state yet
    CHECK(shim_launch_count() == launches0, "a call without a state launched");
    upload(c, p.n);
    const long launches1 = shim_launch_count(), allocs0 = shim_alloc_count();
    const double bad_d[] = {0.0, -1e-9, INFINITY, -INFINITY, NAN};
    for (double b : bad_d) EXPECT(c, amc_init_separate(c, &cfg, b, 1, 1, st), AMC_ERR_INVALID);
    EXPECT(c, amc_init_separate(c, &cfg, d, 0, 1, st), AMC_ERR_INVALID);
    EXPECT(c, amc_init_separate(c, &cfg, d, -1, 1, st), AMC_ERR_INVALID);
    EXPECT(c, amc_init_separate(c, &cfg, d, 1, -1, st), AMC_ERR_INVALID);
    EXPECT(c, amc_init_separate(c, &cfg, d, INT32_MAX, 1, st), AMC_ERR_INVALID);
    EXPECT(c, amc_init_separate(c, &cfg, d, 1 << 30, 1 << 30, st), AMC_ERR_INVALID);
    amc_ic_config bad = cfg;
    bad.struct_size = 8;
    EXPECT(c, amc_init_separate(c, &bad, d, 1, 1, st), AMC_ERR_INVALID);
    bad = cfg;
    bad.n_regions = 9;
    EXPECT(c, amc_init_separate(c, &bad, d, 1, 1, st), AMC_ERR_INVALID);
    bad = cfg;
    bad.n_regions = 1; bad.first[1] = p.n + 1; bad.radius[0] = 1e-8; bad.z_hi[0] = 1e-8;
    EXPECT(c, amc_init_separate(c, &bad, d, 1, 1, st), AMC_ERR_INVALID);        // the regions hold another number of atoms
    CHECK(owned(c) == own0 && shim_launch_count() == launches1 && shim_alloc_count() == allocs0, "a refused call allocated or launched");

    // ---- one search: six launches, the work space given back, statistics written or not asked for -------------------------------------
    for (int k = 0; k < AMC_IC_STATS; k++) st[k] = POISON;
    const long live0 = shim_live_objects();
    OK(c, amc_init_separate(c, &cfg, d, 5, 3, st));
    const long A = shim_alloc_count() - allocs0;
    CHECK(shim_launch_count() - launches1 == 6, "%ld launches in one search (file, two of the scan, scatter, mark, redraw: 6)", shim_launch_count() - launches1);
    CHECK(A >= 9, "%ld allocations in the call", A);
    const int64_t want[AMC_IC_STATS] = {1, 0, 0, 0, 0, 0, 0, 5};
    for (int k = 0; k < AMC_IC_STATS; k++) CHECK(st[k] == want[k], "stats[%d] = %lld", k, (long long)st[k]);
    CHECK(owned(c) == own0 && shim_live_objects() == live0, "the work space was not given back");
    OK(c, amc_init_separate(c, &cfg, d, 1, 0, nullptr));
    {   // a_shape is ignored, and the last round still takes a query
        amc_ic_config g = cfg;
        g.a_shape = -1.0;
        OK(c, amc_init_separate(c, &g, d, INT32_MAX, 0, st));
        CHECK(st[7] == INT32_MAX && st[0] == 1, "a query at the last round");
    }
    for (const char *cells : {"1", "3", "1000", "-4", "x"}) {      // the knob, sane or not: clamped into 1 .. 128
        setenv("AMC_IC_CELLS", cells, 1);
        OK(c, amc_init_separate(c, &cfg, d, 1, 2, st));
        CHECK(st[0] == 1 && owned(c) == own0, "AMC_IC_CELLS=%s", cells);
    }
    unsetenv("AMC_IC_CELLS");
    OK(c, amc_init_separate(c, &cfg, 1.0, 1, 2, st));               // further than the box is wide: one cell
    OK(c, amc_init_separate(c, &cfg, 1e-300, 1, 2, st));            // a square that underflows: the cap of cells
    no_bad_launches("one search");

    // ---- an allocation failure at every allocation of the call ----------------------------------------------------------------------
    for (long k = 1; k <= A; k++) {
        shim_fail_alloc(k);
        for (int q = 0; q < AMC_IC_STATS; q++) st[q] = POISON;
        EXPECT(c, amc_init_separate(c, &cfg, d, 1, 2, st), AMC_ERR_HIP);
        CHECK(shim_alloc_failed() == 1, "allocation %ld of the call was never asked for", k);
        CHECK(owned(c) == own0 && shim_live_objects() == live0, "allocation %ld failed and something of the work space stayed", k);
        CHECK(st[0] == POISON, "statistics written by a failed call");
        shim_fail_alloc(0);
        OK(c, amc_init_separate(c, &cfg, d, 1, 2, st));             // ... and the next call is whole again
    }
    shim_fail_alloc(A + 1);
    OK(c, amc_init_separate(c, &cfg, d, 1, 2, st));
    CHECK(shim_alloc_failed() == 0, "the call made more than A = %ld allocations", A);
    shim_fail_alloc(0);
    printf("A = %ld allocations, every k = 1 .. %ld failed once\n", A, A);
    OK(c, amc_run(c, 1e-12, 2, nullptr));
    amc_destroy(c);
    CHECK(shim_live_objects() == 0, "%ld objects alive after amc_destroy", shim_live_objects());

    // ---- the smallest systems: no launch at all -----------------------------------------------------------------------------------------
    for (int64_t n = 0; n <= 2; n++) {
        p = cube_params(n);
        c = nullptr;
        OK(c, amc_create(&c, &p));
        OK(c, amc_init_synthetic(c, &cfg));
        const int64_t own = owned(c);
        const long l0 = shim_launch_count(), a0 = shim_alloc_count();
        for (int k = 0; k < AMC_IC_STATS; k++) st[k] = POISON;
        OK(c, amc_init_separate(c, &cfg, d, 2, 4, st));
        const int64_t w[AMC_IC_STATS] = {1, 0, 0, 0, 0, 0, 0, 2};
        for (int k = 0; k < AMC_IC_STATS; k++) CHECK(st[k] == w[k], "n = %lld: stats[%d] = %lld", (long long)n, k, (long long)st[k]);
        if (n < 2) CHECK(shim_launch_count() == l0 && shim_alloc_count() == a0, "n = %lld: the call launched or allocated", (long long)n);
        else CHECK(shim_launch_count() - l0 == 6, "n = 2: %ld launches", shim_launch_count() - l0);
        CHECK(owned(c) == own, "n = %lld: the count of owned objects changed", (long long)n);
        OK(c, amc_run(c, 1e-12, 1, nullptr));
        amc_destroy(c);
        CHECK(shim_live_objects() == 0, "%ld objects alive after amc_destroy", shim_live_objects());
    }
    no_bad_launches("the smallest systems");
    printf("ic_separate: ok (%ld allocations, %ld launches)\n", shim_alloc_count(), shim_launch_count());
    return 0;
}
