// driver.cpp — drives the library's host code over the stand-in HIP runtime (hip_shim.cpp) under AddressSanitizer and UBSan.
// Plain C++ against include/argonmc.h; `driver <scenario>` exits non-zero on a wrong return code or wrong content, and the
// sanitizers speak for themselves.  Kernels do not run here (a launch is logged and checked, nothing more): what the scenarios
// see is host-enqueued extents, ownership, error paths, read-backs of memory nobody cleared and launch geometry.
// Every buffer handed to the library is a heap block of exactly its documented size, so a copy that is too long ends in a red zone.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <functional>
#include <string>
#include <vector>

#include "argonmc.h"
#include "hip_shim.h"

// the two runtime calls the liveness scenario makes itself (as the stand-in defines them)
extern "C" int hipMalloc(void **p, size_t bytes);
extern "C" int hipFree(void *p);
extern "C" int hipMemsetAsync(void *dst, int value, size_t bytes, void *stream);

[[noreturn]] static void die()
{
    fflush(stdout);
    fflush(stderr);
    _exit(1);
}
#define FAIL(...)                                                  \
    do {                                                           \
        fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__);       \
        fprintf(stderr, __VA_ARGS__);                              \
        fputc('\n', stderr);                                       \
        die();                                                     \
    } while (0)
#define EXPECT(c, call, want)                                                                                          \
    do {                                                                                                               \
        const int rc_ = (call);                                                                                        \
        if (rc_ != (want)) FAIL("%s returned %d, expected %d: %s", #call, rc_, (int)(want), amc_last_error(c));        \
    } while (0)
#define OK(c, call) EXPECT(c, call, AMC_OK)
#define CHECK(cond, ...) do { if (!(cond)) FAIL(__VA_ARGS__); } while (0)

// ---- buffers of exactly the documented size ---------------------------------------------------------------------------------------
// Prefilled with 0x11: a word the library did not write reads 0x1111..., a word copied from memory nobody cleared 0xA5A5...
template <class T>
struct Buf {
    T *p;
    size_t n;
    explicit Buf(size_t count) : p((T *)malloc(count * sizeof(T))), n(count)
    {
        if (!p) FAIL("out of host memory");
        memset(p, 0x11, n * sizeof(T));
    }
    ~Buf() { free(p); }
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    operator T *() { return p; }
};

static bool all_bytes(const void *q, size_t bytes, unsigned char v)
{
    const unsigned char *b = (const unsigned char *)q;
    for (size_t k = 0; k < bytes; k++)
        if (b[k] != v) return false;
    return bytes != 0;
}
// every element written by the library, none of them from uncleared memory
template <class T>
static void defined(const T *p, size_t n, const char *what)
{
    for (size_t k = 0; k < n; k++) {
        if (all_bytes(p + k, sizeof(T), 0xA5)) FAIL("%s[%zu] reads 0xA5...: memory nobody cleared (a missing memset)", what, k);
        if (sizeof(T) > 1 && all_bytes(p + k, sizeof(T), 0x11)) FAIL("%s[%zu] was not written", what, k);
    }
}
template <class T>
static void defined(const Buf<T> &b, const char *what) { defined(b.p, b.n, what); }
template <class T>
static void zeros(const T *p, size_t n, const char *what)
{
    for (size_t k = 0; k < n; k++)
        if (!all_bytes(p + k, sizeof(T), 0)) {
            defined(p + k, 1, what);
            FAIL("%s[%zu] is not zero before any kernel ran", what, k);
        }
}
template <class T>
static void zeros(const Buf<T> &b, const char *what) { zeros(b.p, b.n, what); }

static void no_bad_launches(const char *where)
{
    const long bad = shim_bad_launch_count();
    for (long k = 0; k < bad && k < 20; k++) fprintf(stderr, "bad launch: %s\n", shim_bad_launch(k));
    if (bad) FAIL("%ld refused launch(es) in %s", bad, where);
}

// ---- contexts ------------------------------------------------------------------------------------------------------------------
// The constants of the three geometries as argon_monte_carlo_amd/params.py forms them (their exact bits do not matter here).
static amc_params make_params(int geometry, int64_t n)
{
    amc_params p;
    memset(&p, 0, sizeof p);
    const double ar = sqrt(3.6e-19 / (4.0 * M_PI));
    p.struct_size = (int32_t)sizeof p;
    p.geometry = geometry;
    p.n = n;
    p.collision_range = 2.0 * ar;
    p.argon_mass = 6.63e-26;
    p.argon_radius = ar;
    p.hist_bins = 200;
    p.hist_lo = 0.0;
    p.hist_hi = 1e-6;
    p.max_paths = 64;
    if (geometry == AMC_GEOM_CELL) {
        p.nx = p.ny = p.nz = 1;
    } else if (geometry == AMC_GEOM_CUBE) {
        p.nx = p.ny = p.nz = 15;
        p.cube_x = p.cube_y = p.cube_z = 100e-9;
        p.dx = p.dy = p.dz = 100e-9 / 15;
        p.overlap_x = p.overlap_y = p.overlap_z = p.dx / 10;
    } else {
        const bool temp = geometry == AMC_GEOM_PORE_ENERGISED;
        const double Rp = 30e-9, Rg = Rp + 4e-9, Hp = 3000e-9, hot = 30e-9, gap = hot, cold = Hp - hot - gap, Roa = 5 * Rp, hoa = 100e-9;
        const double H = Hp + 2 * hoa;
        p.nx = p.ny = 7; p.nz = 148;
        p.dx = p.dy = Roa / 7; p.dz = H / 148;
        p.overlap_x = p.overlap_y = p.overlap_z = p.collision_range;
        p.R_oa = Roa; p.R_p = Rp; p.R_g = Rg;
        p.R_oa_c = Roa - ar; p.R_g_c = Rg - ar; p.R_p_c = Rp - ar;
        p.H = H; p.h_oa = hoa; p.z_cold = H - hoa; p.z_gap_bottom = hoa + hot;
        p.z_gap_top = temp ? hoa + hot + gap : H - hoa - cold;
        p.oob_z_lo_fix = temp ? 50e-9 : 10 * ar;
        p.oob_z_hi_fix = temp ? H - 50e-9 : 10 * ar;
        p.R_oa_sq = Roa * Roa; p.R_g_sq = Rg * Rg; p.R_p_sq = Rp * Rp;
        p.z_oob_hot_top = hoa + hot; p.z_oob_gap_top = hoa + hot + gap;
        if (temp) {
            p.t_z3_cold = H - hoa + ar; p.t_z3_hot = hoa - ar;
            p.t_zgap_lo = p.z_gap_bottom + ar; p.t_zgap_hi = p.z_gap_top - ar;
            p.R_g_c_sq = p.R_g_c * p.R_g_c; p.R_p_c_sq = p.R_p_c * p.R_p_c;
            p.alpha_coated = 0.95; p.alpha_gap = 0.8;
            p.cos85 = cos(85 * M_PI / 180);
        }
    }
    return p;
}
static const char *geometry_name(int g)
{
    static const char *names[] = {"cell", "cube", "pore", "energised pore"};
    return names[g];
}
static bool is_energised(const amc_params &p) { return p.geometry == AMC_GEOM_PORE_ENERGISED; }

// a state inside the geometry (kernels do not run: only the bytes travel)
struct State {
    Buf<double> x, y, z, vx, vy, vz, d, dx, dy, dz;
    Buf<uint8_t> flag;
    explicit State(const amc_params &p) : x(p.n), y(p.n), z(p.n), vx(p.n), vy(p.n), vz(p.n), d(p.n), dx(p.n), dy(p.n), dz(p.n), flag(p.n)
    {
        const bool cube = p.geometry == AMC_GEOM_CUBE || p.geometry == AMC_GEOM_CELL;
        for (int64_t k = 0; k < p.n; k++) {
            const double u = (k + 0.5) / (double)p.n;
            x[k] = cube ? 100e-9 * u : 20e-9 * (u - 0.5);
            y[k] = cube ? 100e-9 * (1 - u) : 20e-9 * (0.5 - u);
            z[k] = cube ? 50e-9 : p.H * u;
            vx[k] = 300.0 * (u - 0.5); vy[k] = 100.0; vz[k] = -250.0 * u;
            d[k] = dx[k] = dy[k] = dz[k] = 1e-9 * u;
            flag[k] = (uint8_t)(k & 1);
        }
    }
    int upload(amc_ctx *c) { return amc_upload(c, x, y, z, vx, vy, vz, d, dx, dy, dz, flag); }
};

static amc_temp_rng make_rng()
{
    amc_temp_rng g;
    memset(&g, 0, sizeof g);
    g.struct_size = (int32_t)sizeof g;
    g.n_gl = 2;
    g.seed = 7;
    g.t_cold = 293.0; g.t_hot = 353.0; g.gap_height = 30e-9; g.gap_bottom_height = 130e-9;
    g.t_debye_alumina = 980.0; g.n_alumina = 10; g.boltzman = 1.38064852e-23;
    g.gl_x[0] = -0.5773502691896257; g.gl_x[1] = 0.5773502691896257;
    g.gl_w[0] = g.gl_w[1] = 1.0;
    return g;
}

static int64_t owned(amc_ctx *c)
{
    int64_t k = -1;
    OK(c, amc_owned_count(c, &k));
    return k;
}

// ---- what the outputs hand back before anything could have run (scenario 4: poison) --------------------------------------------------
static void outputs_defined(amc_ctx *c, const amc_params &p, const char *when)
{
    std::string w = std::string(when) + ": ";
    if (p.hist_bins > 0) {
        Buf<uint64_t> counts((size_t)4 * p.hist_bins);
        uint64_t total = 0x1111111111111111ULL;
        OK(c, amc_histograms(c, counts, &total));
        zeros(counts, (w + "amc_histograms counts").c_str());
        zeros(&total, 1, (w + "amc_histograms n_paths_total").c_str());
    }
    size_t pending = 0x11111111;
    OK(c, amc_paths_pending(c, &pending));
    CHECK(pending == 0, "%samc_paths_pending says %zu before any step", w.c_str(), pending);
    Buf<int64_t> ls(8), os(8);
    OK(c, amc_lists_stats(c, ls));
    defined(ls, (w + "amc_lists_stats").c_str());
    CHECK(ls[5] == 0 && ls[6] == 0, "%samc_lists_stats counts nodes handed out (%lld, %lld) before any kernel ran", w.c_str(), (long long)ls[5], (long long)ls[6]);
    OK(c, amc_overlap_stats(c, os));
    defined(os, (w + "amc_overlap_stats").c_str());
    CHECK(os[1] == 0, "%samc_overlap_stats counts %lld refiled particles before any kernel ran", w.c_str(), (long long)os[1]);
}
static void stats_zero(const amc_step_stats &st, const char *what)
{
    zeros((const int64_t *)&st, sizeof st / sizeof(int64_t), what);
}

// ---- the samplers -------------------------------------------------------------------------------------------------------------------
struct Grids {
    amc_field_grid fields;
    amc_flux_grid flux;
    amc_corr_grid corr;
    amc_mfp_grid mfp;
    amc_vdf_grid vdf;
    amc_transit_grid transit;
    amc_pair_grid pair;
    amc_surface_grid surface;
};
template <class G>
static void box(G &g, const amc_params &p, int n1, int n2, int n3)
{
    g.struct_size = (int32_t)sizeof g;
    g.kind = AMC_FIELDS_CARTESIAN;
    g.n1 = n1; g.n2 = n2; g.n3 = n3;
    const bool cube = p.geometry == AMC_GEOM_CUBE || p.geometry == AMC_GEOM_CELL;
    for (int k = 0; k < 3; k++) { g.lo[k] = cube ? 0.0 : -150e-9; g.hi[k] = cube ? 100e-9 : 150e-9; }
    if (!cube) { g.lo[2] = 0.0; g.hi[2] = p.H; }
}
// big: every sampler at its documented maximum, else one bin / column / zone each
static Grids make_grids(const amc_params &p, bool big, int64_t every)
{
    Grids g;
    memset(&g, 0, sizeof g);
    box(g.fields, p, big ? AMC_FIELDS_MAX_BINS / 8 : 1, big ? 4 : 1, big ? 2 : 1);
    g.fields.every = every;
    box(g.flux, p, big ? AMC_FLUX_MAX_BINS : 1, 1, 1);
    g.flux.every = every;
    box(g.corr, p, big ? AMC_CORR_MAX_GROUPS : 1, 1, 1);
    g.corr.n_lags = big ? AMC_CORR_MAX_CELLS / AMC_CORR_MAX_GROUPS - 1 : 1;
    g.corr.every = every;
    // (free paths: bins * 2 * (7 + hist_bins + 1) columns, at most 6,144)
    box(g.mfp, p, big ? AMC_MFP_MAX_COLUMNS / (2 * (8 + AMC_MFP_MAX_HIST_BINS)) : 1, 1, 1);
    g.mfp.hist_bins = big ? AMC_MFP_MAX_HIST_BINS : 0;
    g.mfp.keep_records = big ? 1 : 0;
    g.mfp.hist_hi = 1e-6;
    box(g.vdf, p, 1, big ? AMC_VDF_MAX_COLUMNS / (4 * AMC_VDF_MAX_HIST_BINS + 8) : 1, 1);
    g.vdf.hist_bins = big ? AMC_VDF_MAX_HIST_BINS : 1;
    g.vdf.every = every;
    g.vdf.v_max = 2000.0;
    g.transit.struct_size = (int32_t)sizeof g.transit;
    g.transit.n_zones = big ? AMC_TRANSIT_MAX_ZONES : 1;
    g.transit.every = every;
    for (int k = 0; k < g.transit.n_zones; k++) { g.transit.axis[k] = k % 3; g.transit.lo[k] = 10e-9 * k; g.transit.hi[k] = 10e-9 * (k + 1); }
    box(g.pair, p, 1, 1, big ? AMC_PAIR_MAX_COLUMNS / (1 + 2 * AMC_PAIR_MAX_HIST_BINS) : 1);
    g.pair.hist_bins = big ? AMC_PAIR_MAX_HIST_BINS : 1;
    g.pair.every = every;
    g.pair.r_max = 5e-9;
    g.surface.struct_size = (int32_t)sizeof g.surface;
    g.surface.nbins = big ? AMC_SURFACE_MAX_BINS : 1;
    for (int s = 0; s < AMC_SURFACE_CASES; s++) { g.surface.lo[s] = 0.0; g.surface.hi[s] = 3.2e-6; }
    return g;
}
static size_t bins_of(int n1, int n2, int n3) { return (size_t)n1 * n2 * n3; }

// the pair sampler needs every shard's final state: in the pore geometries only a context of the whole range has it (argonmc_pair.h)
static bool pair_allowed(amc_ctx *, const amc_params &p, int64_t lo, int64_t hi)
{
    return p.geometry == AMC_GEOM_CUBE || p.geometry == AMC_GEOM_CELL || (lo == 0 && hi == p.n);
}

struct Sampler {
    const char *name;
    std::function<int(amc_ctx *, bool)> config;        // (true: the grid, false: NULL)
    std::function<int(amc_ctx *)> sample;              // (nullptr: events, no manual sample)
    std::function<int(amc_ctx *)> reset;
    std::function<void(amc_ctx *, bool, int64_t)> read_check_load;   // zero: totals must be zero; expected samples (-1: do not check)
    std::function<int(amc_ctx *)> read_off;            // a read with NULL outputs: AMC_ERR_STATE while the sampler is off
};

static std::vector<Sampler> make_samplers(const amc_params &p, const Grids &g, int64_t lo, int64_t hi)
{
    const size_t cnt = (size_t)(hi - lo);
    std::vector<Sampler> v;
    v.push_back({"fields", [&g](amc_ctx *c, bool on) { return amc_fields_config(c, on ? &g.fields : nullptr); }, amc_fields_sample, amc_fields_reset,
                 [&g](amc_ctx *c, bool zero, int64_t want) {
                     Buf<int64_t> t(bins_of(g.fields.n1, g.fields.n2, g.fields.n3) * 14), m(2);
                     OK(c, amc_fields_read(c, t, &m[0], &m[1]));
                     defined(t, "amc_fields_read totals"); defined(m, "amc_fields_read counters");
                     if (zero) { zeros(t, "amc_fields_read totals"); zeros(m, "amc_fields_read counters"); }
                     (void)want;
                     OK(c, amc_fields_load(c, t, m[0], m[1]));
                 },
                 [](amc_ctx *c) { return amc_fields_read(c, nullptr, nullptr, nullptr); }});
    v.push_back({"flux", [&g](amc_ctx *c, bool on) { return amc_flux_config(c, on ? &g.flux : nullptr); }, amc_flux_sample, amc_flux_reset,
                 [&g](amc_ctx *c, bool zero, int64_t) {
                     Buf<int64_t> t(bins_of(g.flux.n1, g.flux.n2, g.flux.n3) * 28), m(2);
                     OK(c, amc_flux_read(c, t, &m[0], &m[1]));
                     defined(t, "amc_flux_read totals"); defined(m, "amc_flux_read counters");
                     if (zero) { zeros(t, "amc_flux_read totals"); zeros(m, "amc_flux_read counters"); }
                     OK(c, amc_flux_load(c, t, m[0], m[1]));
                 },
                 [](amc_ctx *c) { return amc_flux_read(c, nullptr, nullptr, nullptr); }});
    v.push_back({"corr", [&g](amc_ctx *c, bool on) { return amc_corr_config(c, on ? &g.corr : nullptr); }, amc_corr_sample, amc_corr_reset,
                 [&g, cnt](amc_ctx *c, bool zero, int64_t) {
                     Buf<int64_t> t(bins_of(g.corr.n1, g.corr.n2, g.corr.n3) * (size_t)(g.corr.n_lags + 1) * 14), m(4);
                     OK(c, amc_corr_read(c, t, &m[0], &m[1], &m[2], &m[3]));
                     defined(t, "amc_corr_read totals"); defined(m, "amc_corr_read counters");
                     if (zero) { zeros(t, "amc_corr_read totals"); zeros(m, "amc_corr_read counters"); }
                     CHECK(m[3] >= 0 && m[3] <= g.corr.n_lags, "amc_corr_read: window position %lld", (long long)m[3]);
                     Buf<double> x0(cnt), y0(cnt), z0(cnt), vx0(cnt), vy0(cnt), vz0(cnt);
                     OK(c, amc_corr_origin(c, x0, y0, z0, vx0, vy0, vz0));
                     // ("zeros before the first origin", and no kernel stores one here)
                     zeros(x0, "amc_corr_origin x0"); zeros(y0, "amc_corr_origin y0"); zeros(z0, "amc_corr_origin z0");
                     zeros(vx0, "amc_corr_origin vx0"); zeros(vy0, "amc_corr_origin vy0"); zeros(vz0, "amc_corr_origin vz0");
                     OK(c, amc_corr_origin(c, nullptr, nullptr, z0, nullptr, nullptr, nullptr));
                     OK(c, amc_corr_load(c, t, m[0], m[1], m[2], m[3], x0, y0, z0, vx0, vy0, vz0));
                     OK(c, amc_corr_load(c, t, m[0], m[1], m[2], 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
                     OK(c, amc_corr_load(c, t, m[0], m[1], m[2], m[3], x0, y0, z0, vx0, vy0, vz0));
                 },
                 [](amc_ctx *c) { return amc_corr_read(c, nullptr, nullptr, nullptr, nullptr, nullptr); }});
    v.push_back({"mfp", [&g](amc_ctx *c, bool on) { return amc_mfp_config(c, on ? &g.mfp : nullptr); }, nullptr, amc_mfp_reset,
                 [&g](amc_ctx *c, bool zero, int64_t) {
                     const size_t bins = bins_of(g.mfp.n1, g.mfp.n2, g.mfp.n3);
                     Buf<int64_t> t(bins * 28), h(bins * 2 * (size_t)(g.mfp.hist_bins + 1)), m(3);
                     OK(c, amc_mfp_read(c, t, h, &m[0], &m[1], &m[2]));
                     defined(t, "amc_mfp_read totals"); defined(h, "amc_mfp_read hist"); defined(m, "amc_mfp_read counters");
                     if (zero) { zeros(t, "amc_mfp_read totals"); zeros(h, "amc_mfp_read hist"); zeros(m, "amc_mfp_read counters"); }
                     CHECK(m[0] == 0 && m[1] == 0, "amc_mfp_read: %lld records, %lld outside, and no kernel ran", (long long)m[0], (long long)m[1]);
                     OK(c, amc_mfp_load(c, t, h, m[0], m[1], m[2]));
                     if (g.mfp.hist_bins == 0) OK(c, amc_mfp_load(c, t, nullptr, m[0], m[1], m[2]));
                 },
                 [](amc_ctx *c) { return amc_mfp_read(c, nullptr, nullptr, nullptr, nullptr, nullptr); }});
    v.push_back({"vdf", [&g](amc_ctx *c, bool on) { return amc_vdf_config(c, on ? &g.vdf : nullptr); }, amc_vdf_sample, amc_vdf_reset,
                 [&g](amc_ctx *c, bool zero, int64_t) {
                     Buf<int64_t> t(bins_of(g.vdf.n1, g.vdf.n2, g.vdf.n3) * (size_t)(4 * g.vdf.hist_bins + 8)), m(2);
                     OK(c, amc_vdf_read(c, t, &m[0], &m[1]));
                     defined(t, "amc_vdf_read totals"); defined(m, "amc_vdf_read counters");
                     if (zero) { zeros(t, "amc_vdf_read totals"); zeros(m, "amc_vdf_read counters"); }
                     OK(c, amc_vdf_load(c, t, m[0], m[1]));
                 },
                 [](amc_ctx *c) { return amc_vdf_read(c, nullptr, nullptr, nullptr); }});
    v.push_back({"transit", [&g](amc_ctx *c, bool on) { return amc_transit_config(c, on ? &g.transit : nullptr); }, amc_transit_sample, amc_transit_reset,
                 [&g, cnt](amc_ctx *c, bool zero, int64_t) {
                     Buf<int64_t> t((size_t)g.transit.n_zones * AMC_TRANSIT_COLUMNS * 2), m(1);
                     OK(c, amc_transit_read(c, t, &m[0]));
                     defined(t, "amc_transit_read totals"); defined(m, "amc_transit_read n_samples");
                     if (zero) { zeros(t, "amc_transit_read totals"); zeros(m, "amc_transit_read n_samples"); }
                     Buf<uint32_t> state(cnt), entry((size_t)g.transit.n_zones * cnt);
                     OK(c, amc_transit_state(c, state, entry));
                     // (every particle unknown, no entry index: no kernel has looked at one)
                     zeros(state, "amc_transit_state state"); zeros(entry, "amc_transit_state entry");
                     OK(c, amc_transit_state(c, nullptr, entry));
                     OK(c, amc_transit_load(c, t, m[0], state, entry));
                     OK(c, amc_transit_load(c, t, m[0], nullptr, nullptr));
                     OK(c, amc_transit_load(c, t, m[0], state, entry));
                 },
                 [](amc_ctx *c) { return amc_transit_read(c, nullptr, nullptr); }});
    if (pair_allowed(nullptr, p, lo, hi))
        v.push_back({"pair", [&g](amc_ctx *c, bool on) { return amc_pair_config(c, on ? &g.pair : nullptr); }, amc_pair_sample, amc_pair_reset,
                     [&g](amc_ctx *c, bool zero, int64_t) {
                         Buf<int64_t> t(bins_of(g.pair.n1, g.pair.n2, g.pair.n3) * (size_t)(1 + 2 * g.pair.hist_bins)), m(3);
                         OK(c, amc_pair_read(c, t, &m[0], &m[1], &m[2]));
                         defined(t, "amc_pair_read totals"); defined(m, "amc_pair_read counters");
                         if (zero) { zeros(t, "amc_pair_read totals"); zeros(m, "amc_pair_read counters"); }
                         OK(c, amc_pair_load(c, t, m[0], m[1], m[2]));
                     },
                     [](amc_ctx *c) { return amc_pair_read(c, nullptr, nullptr, nullptr, nullptr); }});
    if (is_energised(p))
        v.push_back({"surface", [&g](amc_ctx *c, bool on) { return amc_surface_config(c, on ? &g.surface : nullptr); }, nullptr, amc_surface_reset,
                     [&g](amc_ctx *c, bool zero, int64_t) {
                         Buf<int64_t> t((size_t)AMC_SURFACE_CASES * (size_t)(g.surface.nbins + 1) * 6), f(AMC_SURFACE_CASES), m(1);
                         OK(c, amc_surface_read(c, t, f, &m[0]));
                         defined(t, "amc_surface_read totals"); defined(f, "amc_surface_read n_failed"); defined(m, "amc_surface_read n_steps");
                         zeros(f, "amc_surface_read n_failed");
                         if (zero) { zeros(t, "amc_surface_read totals"); zeros(m, "amc_surface_read n_steps"); }
                         OK(c, amc_surface_load(c, t, f, m[0]));
                     },
                     [](amc_ctx *c) { return amc_surface_read(c, nullptr, nullptr, nullptr); }});
    return v;
}

// ---- steps ----------------------------------------------------------------------------------------------------------------------------
static const double DT = 1e-13;

// one step of the energised pore through the host hand-over, no wall hit (no kernel writes one)
static void energised_handover_step(amc_ctx *c, bool park)
{
    OK(c, amc_temp_begin(c, DT));
    for (int cs = 3; cs <= 9; cs++) {
        Buf<int32_t> idx(1);
        Buf<double> normal(3), cz(1), dir(0), es(0), out(0);
        size_t n = 99;
        OK(c, amc_wall_hits(c, cs, idx, normal, cz, 1, &n));
        CHECK(n == 0, "amc_wall_hits(case %d) reports %zu hits and no kernel ran", cs, n);
        Buf<double> contact(0);
        OK(c, amc_wall_contacts(c, cs, contact, 0));
        if (park && cs == 5) {
            OK(c, amc_wall_park(c, cs, dir, 0));
            OK(c, amc_wall_finish(c, cs, es, 0, out, out));
        } else {
            OK(c, amc_wall_apply(c, cs, dir, es, 0, out, out));
        }
    }
    OK(c, amc_wall_hits_again(c));
    amc_step_stats st;
    memset(&st, 0x11, sizeof st);
    OK(c, amc_temp_end(c, &st));
    stats_zero(st, "amc_temp_end statistics");
}

// what the device-RNG mode hands back, with caller buffers of 0 and 1 records
static void energised_device_reads(amc_ctx *c)
{
    for (size_t cap = 0; cap <= 1; cap++)
        for (int cs = 3; cs <= 9; cs++) {
            Buf<int32_t> idx(cap);
            Buf<double> a(cap), b(cap), n3(3 * cap), d3(3 * cap), c3(3 * cap);
            Buf<uint8_t> ok(cap);
            size_t n = 99;
            OK(c, amc_temp_device_results(c, cs, idx, a, b, ok, cap, &n));
            CHECK(n == 0, "amc_temp_device_results(case %d): %zu hits and no kernel ran", cs, n);
            OK(c, amc_temp_device_draws(c, cs, idx, n3, a, d3, b, cap, &n));
            CHECK(n == 0, "amc_temp_device_draws(case %d): %zu hits and no kernel ran", cs, n);
            OK(c, amc_temp_device_contacts(c, cs, idx, c3, cap, &n));
            CHECK(n == 0, "amc_temp_device_contacts(case %d): %zu hits and no kernel ran", cs, n);
        }
    Buf<double> sums(3);
    Buf<int32_t> had(3);
    OK(c, amc_temp_device_sums(c, sums, had));
    zeros(sums, "amc_temp_device_sums sums");
    zeros(had, "amc_temp_device_sums had");
}

static void energised_device_step(amc_ctx *c, const amc_temp_rng &rng)
{
    OK(c, amc_temp_begin(c, DT));
    OK(c, amc_temp_cases_device(c, &rng));
    amc_step_stats st;
    memset(&st, 0x11, sizeof st);
    OK(c, amc_temp_end(c, &st));
    stats_zero(st, "amc_temp_end statistics");
}

// amc_temp_run_device and the series it leaves: first / count at 0, the last row and one past it.  (The rows themselves are written
// by a kernel: their content is not examined.)
static void energised_run(amc_ctx *c, const amc_temp_rng &rng, int64_t nsteps)
{
    amc_step_stats st;
    memset(&st, 0x11, sizeof st);
    OK(c, amc_temp_run_device(c, DT, nsteps, &rng, &st));
    stats_zero(st, "amc_temp_run_device statistics");
    int64_t rows = -1;
    OK(c, amc_temp_series_read(c, 0, 0, nullptr, nullptr, &rows));
    CHECK(rows == nsteps, "amc_temp_series_read: %lld rows after a run of %lld steps", (long long)rows, (long long)nsteps);
    {
        Buf<double> sums(0);
        Buf<uint8_t> had(0);
        OK(c, amc_temp_series_read(c, 0, 0, sums, had, nullptr));
        OK(c, amc_temp_series_read(c, nsteps, 0, sums, had, nullptr));
        EXPECT(c, amc_temp_series_read(c, nsteps + 1, 0, sums, had, nullptr), AMC_ERR_INVALID);
    }
    if (nsteps > 0) {
        Buf<double> sums(3), all((size_t)3 * nsteps);
        Buf<uint8_t> had(3), hall((size_t)3 * nsteps);
        OK(c, amc_temp_series_read(c, nsteps - 1, 1, sums, had, nullptr));
        OK(c, amc_temp_series_read(c, 0, nsteps, all, hall, nullptr));
        EXPECT(c, amc_temp_series_read(c, nsteps, 1, sums, had, nullptr), AMC_ERR_INVALID);
        EXPECT(c, amc_temp_series_read(c, nsteps - 1, 2, sums, had, nullptr), AMC_ERR_INVALID);
    }
    energised_device_reads(c);
}

// ---- scenario 1: the lifetime of one context of every kind ---------------------------------------------------------------------------------
static void lifetime_one(int geometry, int64_t n, int detect_mode, int reserved0, int64_t max_paths)
{
    amc_params p = make_params(geometry, n);
    p.detect_mode = detect_mode;
    p.reserved0 = reserved0;
    p.max_paths = max_paths;
    amc_ctx *c = nullptr;
    if (amc_create(&c, &p) != AMC_OK) FAIL("amc_create(%s, n=%lld): %s", geometry_name(geometry), (long long)n, amc_last_error(nullptr));
    outputs_defined(c, p, "after amc_create");
    const int64_t owned0 = owned(c);
    State s(p);
    OK(c, s.upload(c));
    OK(c, amc_upload(c, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
    amc_step_stats st;
    const amc_temp_rng rng = make_rng();
    if (!is_energised(p)) {
        memset(&st, 0x11, sizeof st);
        OK(c, amc_timestep(c, DT, &st));
        stats_zero(st, "amc_timestep statistics");
        memset(&st, 0x11, sizeof st);
        OK(c, amc_run(c, DT, 9, &st));
        stats_zero(st, "amc_run statistics");
        OK(c, amc_run(c, DT, 0, nullptr));
        if (geometry != AMC_GEOM_CELL) {
            int64_t moved = 0x1111;
            OK(c, amc_stage_drift(c, DT));
            OK(c, amc_stage_walls(c, &st));
            OK(c, amc_stage_bounds(c, &moved));
            CHECK(moved == 0, "amc_stage_bounds moved %lld particles and no kernel ran", (long long)moved);
        }
        OK(c, amc_stage_sweep(c, &st));
        EXPECT(c, amc_temp_begin(c, DT), AMC_ERR_STATE);
    } else {
        EXPECT(c, amc_run(c, DT, 9, &st), AMC_ERR_INVALID);
        energised_handover_step(c, false);
        energised_handover_step(c, true);
        energised_device_step(c, rng);
        energised_device_reads(c);
        energised_run(c, rng, 0);
        energised_run(c, rng, 3);
        energised_run(c, rng, 5);       // (the series grows)
        energised_run(c, rng, 2);
    }
    {
        State back(p);
        OK(c, amc_download(c, back.x, back.y, back.z, back.vx, back.vy, back.vz, back.d, back.dx, back.dy, back.dz, back.flag));
        CHECK(!n || !memcmp(back.x.p, s.x.p, sizeof(double) * (size_t)n), "amc_download x differs from what was uploaded and no kernel ran");
        CHECK(!n || !memcmp(back.flag.p, s.flag.p, (size_t)n), "amc_download flags differ from what was uploaded and no kernel ran");
        OK(c, amc_download(c, nullptr, nullptr, back.z, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
        Buf<double> px(n), py(n), pz(n);
        if ((reserved0 & 1) || is_energised(p)) {      // (an energised step keeps prior_*_vals on its own)
            OK(c, amc_download_prior(c, px, py, pz));
            defined(px, "amc_download_prior px"); defined(py, "amc_download_prior py"); defined(pz, "amc_download_prior pz");
        } else {
            EXPECT(c, amc_download_prior(c, px, py, pz), AMC_ERR_STATE);
        }
    }
    outputs_defined(c, p, "after the steps");
    {
        Buf<amc_path_record> rec(2);
        size_t got = 99;
        OK(c, amc_drain_paths(c, rec, 2, &got));
        CHECK(got == 0, "amc_drain_paths returns %zu records and no kernel ran", got);
        Buf<amc_path_record> none(0);
        OK(c, amc_drain_paths(c, none, 0, &got));
    }
    OK(c, amc_reset_outputs(c));
    outputs_defined(c, p, "after amc_reset_outputs");
    {
        amc_ic_config ic;
        memset(&ic, 0, sizeof ic);
        ic.struct_size = (int32_t)sizeof ic;
        ic.seed = 5; ic.a_shape = 250.0;
        if (geometry == AMC_GEOM_PORE || is_energised(p)) {
            ic.n_regions = 2;
            ic.first[1] = n / 2; ic.first[2] = n;
            ic.radius[0] = ic.radius[1] = 20e-9; ic.z_hi[0] = ic.z_lo[1] = 1e-6; ic.z_hi[1] = 2e-6;
        }
        OK(c, amc_init_synthetic(c, &ic));
    }
    int fake_stream;
    OK(c, amc_set_stream(c, &fake_stream));
    OK(c, amc_synchronize(c));
    OK(c, amc_set_stream(c, nullptr));
    OK(c, amc_use_null_stream(c));
    OK(c, amc_set_stream(c, nullptr));
    OK(c, amc_profile(c, 1));
    if (!is_energised(p)) OK(c, amc_timestep(c, DT, &st));
    else energised_device_step(c, rng);
    {
        Buf<double> ms(AMC_K_COUNT);
        Buf<int64_t> launches(AMC_K_COUNT);
        OK(c, amc_kernel_times(c, ms, launches));
        defined(ms, "amc_kernel_times total_ms"); defined(launches, "amc_kernel_times launches");
    }
    OK(c, amc_profile(c, 0));
    // every sampler on and off again: the context owns what it owned before (plus the profiling events and what the steps allocate lazily)
    const int64_t owned1 = owned(c);
    CHECK(owned1 >= owned0, "amc_owned_count fell from %lld to %lld", (long long)owned0, (long long)owned1);
    const Grids g = make_grids(p, false, 2);
    std::vector<Sampler> S = make_samplers(p, g, 0, n);
    for (auto &sm : S) {
        if (!strcmp(sm.name, "mfp") && max_paths < 0) { EXPECT(c, sm.config(c, true), AMC_ERR_STATE); continue; }
        OK(c, sm.config(c, true));
    }
    CHECK(owned(c) > owned1, "amc_owned_count did not grow with the samplers on");
    for (auto &sm : S) OK(c, sm.config(c, false));
    CHECK(owned(c) == owned1, "amc_owned_count is %lld after every sampler was switched off, %lld before any config", (long long)owned(c), (long long)owned1);
    for (auto &sm : S) EXPECT(c, sm.read_off(c), AMC_ERR_STATE);
    amc_destroy(c);
    CHECK(shim_live_objects() == 0, "%ld objects alive after amc_destroy", shim_live_objects());
}

static const int64_t SIZES[] = {0, 1, 2, 1001};

static void scenario_lifetime()
{
    for (int64_t n : SIZES) {
        lifetime_one(AMC_GEOM_CELL, n, 0, 0, 64);
        lifetime_one(AMC_GEOM_CELL, n, 2, 1, -1);
        for (int g = AMC_GEOM_CUBE; g <= AMC_GEOM_PORE_ENERGISED; g++) {
            lifetime_one(g, n, 1, 0, 64);
            lifetime_one(g, n, 2, 1, -1);
            lifetime_one(g, n, 0, 1, 64);
        }
    }
    lifetime_one(AMC_GEOM_CUBE, 1001, 0, 0, 0);        // (the default record buffer, once)
    // what amc_create refuses
    amc_ctx *c = (amc_ctx *)&c;
    amc_params p = make_params(AMC_GEOM_CELL, 4);
    p.detect_mode = 1;
    CHECK(amc_create(&c, &p) == AMC_ERR_INVALID && !c && strlen(amc_last_error(nullptr)), "amc_create(cell, detect_mode 1) was not refused");
    p = make_params(AMC_GEOM_CUBE, 4);
    p.fine_cell = 1e-12;
    CHECK(amc_create(&c, &p) == AMC_ERR_INVALID && !c && strlen(amc_last_error(nullptr)), "amc_create(fine_cell too small) was not refused");
    p = make_params(AMC_GEOM_CUBE, 4);
    p.device = 1;
    CHECK(amc_create(&c, &p) == AMC_ERR_NO_DEVICE && !c, "amc_create(device 1) was not refused");
    CHECK(shim_live_objects() == 0, "%ld objects alive after refused amc_create calls", shim_live_objects());
}

// ---- scenario 2: every sampler ------------------------------------------------------------------------------------------------------------
static void samplers_one(int geometry, int64_t n, int64_t lo, int64_t hi, bool big)
{
    amc_params p = make_params(geometry, n);
    amc_ctx *c = nullptr;
    if (amc_create(&c, &p) != AMC_OK) FAIL("amc_create(%s, n=%lld): %s", geometry_name(geometry), (long long)n, amc_last_error(nullptr));
    const bool whole = lo == 0 && hi == n;
    if (!whole) OK(c, amc_set_shard(c, lo, hi));
    State s(p);
    OK(c, s.upload(c));
    const Grids g = make_grids(p, big, 2), g2 = make_grids(p, !big, 3);
    std::vector<Sampler> S = make_samplers(p, g, lo, hi), S2 = make_samplers(p, g2, lo, hi);
    if (!pair_allowed(c, p, lo, hi)) EXPECT(c, amc_pair_config(c, &g.pair), AMC_ERR_STATE);
    const amc_temp_rng rng = make_rng();
    if (is_energised(p)) {      // (the energised steps build their work spaces at the first call: before the count is taken)
        energised_device_step(c, rng);
        energised_handover_step(c, true);
        if (whole) energised_run(c, rng, 5);
    }
    const int64_t owned0 = owned(c);
    for (size_t k = 0; k < S.size(); k++) {
        EXPECT(c, S[k].read_off(c), AMC_ERR_STATE);
        OK(c, S2[k].config(c, true));       // (another grid first: the second config replaces its buffers)
        OK(c, S[k].config(c, true));
        S[k].read_check_load(c, true, 0);   // (poison: a new grid starts from zero totals)
        if (S[k].sample) OK(c, S[k].sample(c));
    }
    amc_step_stats st;
    if (!is_energised(p)) {
        OK(c, amc_timestep(c, DT, &st));
        OK(c, amc_run(c, DT, 5, &st));
        OK(c, amc_run(c, DT, 9, nullptr));
    } else {
        for (int k = 0; k < 3; k++) energised_device_step(c, rng);
        energised_handover_step(c, true);
        if (whole) energised_run(c, rng, 5);
    }
    for (auto &sm : S) {
        sm.read_check_load(c, false, -1);
        OK(c, sm.reset(c));
        sm.read_check_load(c, true, 0);
    }
    OK(c, amc_reset_outputs(c));            // (leaves the samplers alone)
    for (size_t k = 0; k < S.size(); k += 2) OK(c, S[k].config(c, false));
    for (size_t k = 0; k < S.size(); k += 2) EXPECT(c, S[k].read_off(c), AMC_ERR_STATE);
    if (!is_energised(p)) OK(c, amc_timestep(c, DT, &st));
    else energised_device_step(c, rng);
    for (size_t k = 0; k < S.size(); k += 2) OK(c, S[k].config(c, true));
    for (size_t k = 0; k < S.size(); k++) OK(c, S[k].config(c, false));
    CHECK(owned(c) == owned0, "amc_owned_count is %lld with every sampler off, %lld before any config", (long long)owned(c), (long long)owned0);
    for (size_t k = 0; k < S.size(); k++) OK(c, S[k].config(c, true));
    amc_destroy(c);                          // (with the samplers still on)
    CHECK(shim_live_objects() == 0, "%ld objects alive after amc_destroy", shim_live_objects());
}

static void scenario_samplers()
{
    for (int g = AMC_GEOM_CUBE; g <= AMC_GEOM_PORE_ENERGISED; g++)
        for (int64_t n : SIZES)
            for (int big = 0; big <= 1; big++) {
                samplers_one(g, n, 0, n, big != 0);
                if (n >= 1) samplers_one(g, n, 1, n, big != 0);
                if (n >= 2) samplers_one(g, n, 1, n - 1, big != 0);
            }
}

// ---- scenario 3: the sharded step -----------------------------------------------------------------------------------------------------------
static void shard_of(int64_t n, int world, int rank, int64_t *lo, int64_t *hi)
{
    const int64_t base = n / world, rem = n % world;
    *lo = rank * base + (rank < rem ? rank : rem);
    *hi = *lo + base + (rank < rem ? 1 : 0);
}
// write and read the whole documented extent of a view
template <class T>
static void touch(void *view, size_t count, const char *what)
{
    CHECK(view != nullptr, "%s is null", what);
    volatile unsigned char *q = (volatile unsigned char *)view;
    const size_t bytes = count * sizeof(T);
    unsigned int acc = 0;
    for (size_t k = 0; k < bytes; k++) { acc += q[k]; q[k] = (unsigned char)k; }
    for (size_t k = 0; k < bytes; k++) acc += q[k];
    volatile unsigned int sink = acc;
    (void)sink;
}

static void sharded_one(int geometry, int64_t n, int world, int rank)
{
    amc_params p = make_params(geometry, n);
    p.detect_mode = 1;
    amc_ctx *c = nullptr;
    if (amc_create(&c, &p) != AMC_OK) FAIL("amc_create(%s, n=%lld): %s", geometry_name(geometry), (long long)n, amc_last_error(nullptr));
    int64_t lo, hi;
    shard_of(n, world, rank, &lo, &hi);
    OK(c, amc_set_shard(c, lo, hi));
    State s(p);
    OK(c, s.upload(c));
    void *send = nullptr, *recv = nullptr;
    int64_t block = 0;
    // (another world size first: the view is replaced)
    OK(c, amc_mg_exchange_view(c, world + 1, &send, &recv, &block));
    touch<double>(send, (size_t)block, "exchange send"); touch<double>(recv, (size_t)block * (size_t)(world + 1), "exchange recv");
    OK(c, amc_mg_exchange_view(c, world, &send, &recv, &block));
    {
        const int64_t m = std::max<int64_t>((n + world - 1) / world, 1), cap = std::max<int64_t>(4096, m / 8);
        CHECK(block == 3 * m + 16 + 4 * cap, "amc_mg_exchange_view: block of %lld doubles, documented 3 m + 16 + 4 cap = %lld", (long long)block, (long long)(3 * m + 16 + 4 * cap));
    }
    touch<double>(send, (size_t)block, "exchange send"); touch<double>(recv, (size_t)block * (size_t)world, "exchange recv");
    void *csend = nullptr, *crecv = nullptr;
    int64_t cints = 0;
    OK(c, amc_mg_candidates_view(c, world + 1, &csend, &crecv, &cints));
    OK(c, amc_mg_candidates_view(c, world, &csend, &crecv, &cints));
    CHECK(cints >= 2 + 2 * 4096, "amc_mg_candidates_view: %lld integers per block", (long long)cints);
    touch<int32_t>(csend, (size_t)cints, "candidates send"); touch<int32_t>(crecv, (size_t)cints * (size_t)world, "candidates recv");
    amc_step_stats st;
    const amc_temp_rng rng = make_rng();
    if (!is_energised(p)) {
        for (int k = 0; k < 5; k++) {
            OK(c, amc_mg_local(c, DT));
            OK(c, amc_mg_bounds(c));
            OK(c, amc_mg_pack(c, world));
            EXPECT(c, amc_timestep(c, DT, &st), AMC_ERR_STATE);
            OK(c, amc_mg_sweep(c, world, rank));
            memset(&st, 0x11, sizeof st);
            OK(c, amc_mg_finish(c, k & 1 ? &st : nullptr));
            if (k & 1) stats_zero(st, "amc_mg_finish statistics");
        }
        for (int k = 0; k < 5; k++) {
            OK(c, amc_mg_local(c, DT));
            OK(c, amc_mg_bounds(c));
            OK(c, amc_mg_pack(c, world));
            OK(c, amc_mg_detect(c, world, rank));
            OK(c, amc_mg_resolve(c, world));
            OK(c, amc_mg_finish(c, &st));
        }
    } else {
        // the device-RNG step over shards, with the hits exchange (argonmc_shard.h)
        void *hsend = nullptr, *hrecv = nullptr;
        int64_t words = 0;
        for (int w : {64, world}) {
            OK(c, amc_mg_hits_view(c, w, &hsend, &hrecv, &words));
            const int64_t Hc = std::max<int64_t>(512, n / 2048 + 512);
            CHECK(words == 8 + 7 * 3 * Hc, "amc_mg_hits_view: block of %lld words, documented 8 + 7 * 3 * Hc = %lld", (long long)words, (long long)(8 + 21 * Hc));
            touch<int64_t>(hsend, (size_t)words, "hits send"); touch<int64_t>(hrecv, (size_t)words * (size_t)w, "hits recv");
        }
        EXPECT(c, amc_mg_hits_view(c, 65, &hsend, &hrecv, &words), AMC_ERR_INVALID);
        for (int form = 0; form < 2; form++) {
            OK(c, amc_temp_shard_run_begin(c, 5));
            for (int k = 0; k < 5; k++) {
                OK(c, amc_temp_begin(c, DT));
                OK(c, amc_temp_cases_device(c, &rng));
                OK(c, amc_mg_hits_pack(c, world));
                OK(c, amc_mg_hits_sums(c, world, k));
                OK(c, amc_mg_bounds(c));
                OK(c, amc_mg_pack(c, world));
                if (form == 0) OK(c, amc_mg_sweep(c, world, rank));
                else { OK(c, amc_mg_detect(c, world, rank)); OK(c, amc_mg_resolve(c, world)); }
                OK(c, amc_mg_finish(c, nullptr));
            }
            memset(&st, 0x11, sizeof st);
            OK(c, amc_temp_shard_run_end(c, 5, &st));
            stats_zero(st, "amc_temp_shard_run_end statistics");
            Buf<double> sums(15);
            Buf<uint8_t> had(15);
            int64_t rows = -1;
            OK(c, amc_temp_series_read(c, 0, 5, sums, had, &rows));
            CHECK(rows == 5, "amc_temp_series_read: %lld rows after a sharded run of 5 steps", (long long)rows);
            EXPECT(c, amc_temp_series_read(c, 5, 1, sums, had, nullptr), AMC_ERR_INVALID);
        }
    }
    outputs_defined(c, p, "after the sharded steps");
    amc_destroy(c);
    CHECK(shim_live_objects() == 0, "%ld objects alive after amc_destroy", shim_live_objects());
}

static void scenario_sharded()
{
    for (int g = AMC_GEOM_CUBE; g <= AMC_GEOM_PORE_ENERGISED; g++)
        for (int64_t n : SIZES) {
            sharded_one(g, n, 1, 0);
            for (int r = 0; r < 3; r++) sharded_one(g, n, 3, r);        // (n = 2: rank 2's shard is empty)
            sharded_one(g, n, 4, 1);
            sharded_one(g, n, 4, 3);
        }
    sharded_one(AMC_GEOM_PORE_ENERGISED, 1001, 64, 63);
    sharded_one(AMC_GEOM_CUBE, 1001, 64, 17);
}

// ---- scenario 5: every allocation of a set-up fails once --------------------------------------------------------------------------------------
struct Step {
    const char *name;
    std::function<int(amc_ctx *)> run;
    std::function<int(amc_ctx *)> off;      // (samplers) a read that must say AMC_ERR_STATE after a failed config; else nullptr
    bool staged = false;                    // the call builds two work spaces one after the other: the first stays when the second fails
};

// One pass of "create + shard + upload + every sampler + the set-up of a sharded step".  fail_at > 0: that allocation fails.
// Returns the allocations the pass asked for.
static long setup_pass(int geometry, int64_t n, long fail_at, int *n_tolerated)
{
    amc_params p = make_params(geometry, n);
    if (geometry != AMC_GEOM_CELL) p.detect_mode = 1;
    const Grids g = make_grids(p, false, 2);
    const amc_temp_rng rng = make_rng();
    State s(p);
    static void *v[2];
    static int64_t words;
    std::vector<Step> steps;
    steps.push_back({"amc_set_shard", [n](amc_ctx *c) { return amc_set_shard(c, 0, n); }, nullptr});
    steps.push_back({"amc_upload", [&s](amc_ctx *c) { return s.upload(c); }, nullptr});
    std::vector<Sampler> S = make_samplers(p, g, 0, n);
    for (auto &sm : S) steps.push_back({sm.name, [&sm](amc_ctx *c) { return sm.config(c, true); }, sm.read_off});
    steps.push_back({"amc_mg_exchange_view", [](amc_ctx *c) { return amc_mg_exchange_view(c, 3, &v[0], &v[1], &words); }, nullptr});
    steps.push_back({"amc_mg_candidates_view", [](amc_ctx *c) { return amc_mg_candidates_view(c, 3, &v[0], &v[1], &words); }, nullptr});
    if (is_energised(p)) {
        steps.push_back({"amc_temp_begin", [](amc_ctx *c) { return amc_temp_begin(c, DT); }, nullptr});
        steps.push_back({"amc_temp_cases_device", [&rng](amc_ctx *c) { return amc_temp_cases_device(c, &rng); }, nullptr});
        steps.push_back({"amc_temp_shard_run_begin", [](amc_ctx *c) { return amc_temp_shard_run_begin(c, 4); }, nullptr, true});
        steps.push_back({"amc_mg_hits_view", [](amc_ctx *c) { return amc_mg_hits_view(c, 3, &v[0], &v[1], &words); }, nullptr});
        steps.push_back({"amc_temp_run_device", [&rng](amc_ctx *c) { return amc_temp_run_device(c, DT, 6, &rng, nullptr); }, nullptr, true});
    } else if (geometry != AMC_GEOM_CELL) {
        steps.push_back({"amc_mg_local", [](amc_ctx *c) { return amc_mg_local(c, DT); }, nullptr});
    }

    const long before = shim_alloc_count();
    shim_fail_alloc(fail_at);
    int failures = 0;
    amc_ctx *c = (amc_ctx *)&c;
    int rc = amc_create(&c, &p);
    const bool failed_in_create = shim_alloc_failed() != 0;
    if (rc != AMC_OK) {
        failures++;
        CHECK(fail_at > 0 && shim_alloc_failed(), "amc_create(%s) failed on its own: %s", geometry_name(geometry), amc_last_error(nullptr));
        CHECK(c == nullptr, "a failed amc_create left a context");
        CHECK(rc == AMC_ERR_HIP && strlen(amc_last_error(nullptr)) > 0, "a failed amc_create returned %d with the message '%s'", rc, amc_last_error(nullptr));
        CHECK(shim_live_objects() == 0, "%ld objects alive after a failed amc_create", shim_live_objects());
        OK(c, amc_create(&c, &p));          // (and the next one works)
    }
    for (auto &st : steps) {
        const int64_t owned0 = owned(c);
        const bool had_failed = shim_alloc_failed();
        rc = st.run(c);
        if (rc != AMC_OK) {
            failures++;
            CHECK(fail_at > 0 && shim_alloc_failed() && !had_failed, "%s failed on its own (%d): %s", st.name, rc, amc_last_error(c));
            CHECK(rc == AMC_ERR_HIP && strlen(amc_last_error(c)) > 0, "%s: a failed allocation returned %d with the message '%s'", st.name, rc, amc_last_error(c));
            // (all or nothing, but for a work space an earlier stage of the same call has completed: it is kept and used)
            CHECK(st.staged ? owned(c) >= owned0 : owned(c) == owned0, "%s: amc_owned_count is %lld after the failure, %lld before the call", st.name, (long long)owned(c), (long long)owned0);
            if (st.off) EXPECT(c, st.off(c), AMC_ERR_STATE);       // (a failed config leaves the sampler off)
            OK(c, st.run(c));               // (the context is still usable: the same call now succeeds)
        }
    }
    if (fail_at > 0) {
        CHECK(shim_alloc_failed(), "allocation %ld of the pass was never asked for", fail_at);
        // amc_create goes on without its two PINNED buffers (the host-mapped words of the launch plans, the staging buffer of
        // the small read-backs: amc_stage then copies directly and amc_run keeps the ordered workgroup in every sweep).  Every
        // other failed allocation is an error of the call that asked for it.
        const bool tolerated = failures == 0 && shim_alloc_failed() == 2 && failed_in_create;
        CHECK(failures == 1 || tolerated, "allocation %ld failed and %d calls returned an error", fail_at, failures);
        if (tolerated) {
            *n_tolerated += 1;
            outputs_defined(c, p, "without a pinned buffer");
            if (!is_energised(p)) OK(c, amc_run(c, DT, 9, nullptr));
        }
    }
    shim_fail_alloc(0);
    // still usable: a step, then everything goes
    amc_step_stats stt;
    if (is_energised(p)) energised_device_step(c, rng);
    else OK(c, amc_timestep(c, DT, &stt));
    const long asked = shim_alloc_count() - before;
    amc_destroy(c);
    CHECK(shim_live_objects() == 0, "%ld objects alive after amc_destroy", shim_live_objects());
    return asked;
}

static void scenario_alloc_sweep()
{
    for (int g = AMC_GEOM_CELL; g <= AMC_GEOM_PORE_ENERGISED; g++)
        for (int64_t n : {(int64_t)1001, (int64_t)0}) {        // (the empty system allocates the same objects, one element each)
            int tolerated = 0;
            const long A = setup_pass(g, n, 0, &tolerated);
            CHECK(A > 10, "%s: a pass of %ld allocations", geometry_name(g), A);
            for (long k = 1; k <= A; k++) setup_pass(g, n, k, &tolerated);
            CHECK(tolerated == 2, "%s: amc_create went on without %d allocations (its two pinned buffers are optional, nothing else)", geometry_name(g), tolerated);
            printf("allocation-failure sweep, %s, n = %lld: A = %ld allocations, every k = 1 .. %ld failed once (%d of them pinned buffers amc_create does without)\n",
                   geometry_name(g), (long long)n, A, A, tolerated);
        }
}

// ---- scenario 6: the empty system with every sampler on a cadence ------------------------------------------------------------------------------
static void scenario_empty_samplers()
{
    for (int geometry : {AMC_GEOM_CUBE, AMC_GEOM_PORE}) {
        amc_params p = make_params(geometry, 0);
        amc_ctx *c = nullptr;
        OK(c, amc_create(&c, &p));
        State s(p);
        OK(c, s.upload(c));
        const Grids g = make_grids(p, false, 2);
        std::vector<Sampler> S = make_samplers(p, g, 0, 0);
        for (auto &sm : S) OK(c, sm.config(c, true));
        amc_step_stats st;
        int rc = AMC_OK;        // (the first failure; the steps go on, so that the launch log is complete)
        for (int k = 0; k < 10; k++)
            if (const int r = amc_timestep(c, DT, &st); r != AMC_OK && rc == AMC_OK) rc = r;
        if (const int r = amc_run(c, DT, 10, &st); r != AMC_OK && rc == AMC_OK) rc = r;
        printf("%s, n = 0, every sampler at every = 2: %ld launches of k_pair_file, %ld of k_pair_scatter\n", geometry_name(geometry),
               shim_launches_of("k_pair_file"), shim_launches_of("k_pair_scatter"));
        no_bad_launches("the empty system with every sampler on");
        CHECK(rc == AMC_OK, "a step of the empty system returned %d: %s", rc, amc_last_error(c));
        amc_destroy(c);
    }
}

// ---- scenario 7: is the sanitizer live in what was built? -----------------------------------------------------------------------------------------
static void scenario_liveness()
{
    void *p = nullptr;
    if (hipMalloc(&p, 64) != 0) FAIL("the stand-in's hipMalloc failed");
    hipMemsetAsync(p, 0, 72, nullptr);      // eight bytes past the block: AddressSanitizer must end the run here
    hipFree(p);
    printf("the overrun went unnoticed\n");
}

int main(int argc, char **argv)
{
    const std::string name = argc > 1 ? argv[1] : "";
    const struct { const char *name; void (*run)(); } scenarios[] = {
        {"lifetime", scenario_lifetime}, {"samplers", scenario_samplers}, {"sharded", scenario_sharded},
        {"alloc_sweep", scenario_alloc_sweep}, {"empty_samplers", scenario_empty_samplers}, {"liveness", scenario_liveness},
    };
    for (const auto &s : scenarios)
        if (name == s.name) {
            s.run();
            no_bad_launches(s.name);
            printf("%s: ok (%ld allocations, %ld launches)\n", s.name, shim_alloc_count(), shim_launch_count());
            return 0;
        }
    fprintf(stderr, "usage: driver lifetime | samplers | sharded | alloc_sweep | empty_samplers | liveness\n");
    return 2;
}
