// amc_api_temp.hip — C ABI of the energised-wall path (Temperature_Pore_MC.py, Temp:662-853): the per-case hand-over to
// the host's random draws (amc_wall_hits / amc_wall_apply) and the opt-in device-side sampling (amc_temp_cases_device).
#include "amc_case_sums_dev.h"
#include "amc_host.h"

extern "C" {

// ---- energised walls (Temp) ---------------------------------------------------------------------------------------------
static int temp_ensure(amc_ctx *c)
{
    if (c->P.geometry != AMC_GEOM_PORE_ENERGISED) return amc_fail(c, AMC_ERR_STATE, "energised-wall calls need AMC_GEOM_PORE_ENERGISED");
    if (c->T.idx) return AMC_OK;
    amc_alloc_group group(c);
    const int icap = (int)std::min<int64_t>(std::max<int64_t>(4096, c->n / 8 + 1024), 0x3fffffff);
    const size_t cap = (size_t)icap;
    // one pinned, device-mapped block: [count | idx | t | contact | normal | dir | Es | dpz | dE | ok]
    size_t off = 0;
    auto place = [&](size_t bytes) { const size_t at = off; off = (off + bytes + 255) & ~(size_t)255; return at; };
    const size_t o_count = place(64), o_idx = place(sizeof(int) * cap), o_t = place(sizeof(double) * cap),
                 o_contact = place(sizeof(double) * 3 * cap), o_normal = place(sizeof(double) * 3 * cap),
                 o_dir = place(sizeof(double) * 3 * cap), o_Es = place(sizeof(double) * cap), o_dpz = place(sizeof(double) * cap),
                 o_dE = place(sizeof(double) * cap), o_ok = place(cap), o_dEs = place(sizeof(double) * cap),
                 o_ddpz = place(sizeof(double) * cap), o_ddE = place(sizeof(double) * cap);
    void *hp, *dp = nullptr;
    int *count, *def_idx;
    double *def_dir;
    AMC_HIP(c, palloc(c, &hp, off, hipHostMallocMapped));
    AMC_HIP(c, hipHostGetDevicePointer(&dp, hp, 0));
    AMC_HIP(c, dalloc(c, &count, 16));      // (the hit counter stays in device memory: every hit increments it atomically)
    AMC_HIP(c, dalloc(c, &def_idx, cap));
    AMC_HIP(c, dalloc(c, &def_dir, 3 * cap));
    group.keep();
    memset(hp, 0, off);
    amc_temp_ws &T = c->T;
    char *h = (char *)hp, *d = (char *)dp;
    T.cap = icap; T.pin = hp; T.count = count; T.def_idx = def_idx; T.def_dir = def_dir;
    T.t = (double *)(d + o_t); T.contact = (double *)(d + o_contact);
    T.normal = (double *)(d + o_normal); T.dir = (double *)(d + o_dir); T.Es = (double *)(d + o_Es); T.dpz = (double *)(d + o_dpz);
    T.dE = (double *)(d + o_dE); T.ok = (unsigned char *)(d + o_ok);
    T.h_count = (int *)(h + o_count); T.h_idx = (int *)(h + o_idx); T.h_contact = (double *)(h + o_contact);
    T.h_normal = (double *)(h + o_normal); T.h_dir = (double *)(h + o_dir); T.h_Es = (double *)(h + o_Es);
    T.h_dpz = (double *)(h + o_dpz); T.h_dE = (double *)(h + o_dE);
    T.def_Es = (double *)(d + o_dEs); T.def_dpz = (double *)(d + o_ddpz); T.def_dE = (double *)(d + o_ddE);
    T.h_def_Es = (double *)(h + o_dEs); T.h_def_dpz = (double *)(h + o_ddpz); T.h_def_dE = (double *)(h + o_ddE);
    T.idx = (int *)(d + o_idx);             // (the guard: last)
    return AMC_OK;
}

int amc_temp_begin(amc_ctx *c, double dt)
{
    if (!c || !c->uploaded) return AMC_ERR_STATE;
    AMC_HIP(c, hipSetDevice(c->device));
    int rc = temp_ensure(c);
    if (rc) return rc;
    if ((rc = amc_flush(c))) return rc;
    c->keep_prior = true;       // the energised masks read prior_*_vals (Temp:708-750)
    c->T.h.fresh();
    amc_mg_step_fresh(c);
    AMC_HIP(c, amc_launch_stream(c, dt, AMC_ST_DRIFT | AMC_ST_WALLS, 0));
    return AMC_OK;
}

// sorted position -> record, ascending particle index (unique: a particle hits a case at most once per step)
static void temp_order(const int *idx, size_t n, std::vector<int> &perm)
{
    perm.resize(n);
    for (size_t k = 0; k < n; k++) perm[k] = (int)k;
    std::sort(perm.begin(), perm.end(), [idx](int a, int b) { return idx[a] < idx[b]; });
}

// The hits of `case_id` (none past the last case) behind whatever is enqueued, their count, ONE synchronisation.  A case's
// mask is evaluated on the state the previous apply leaves (Temp:708-751) and needs nothing from the host: behind that kernel,
// one synchronisation returns its results and this case's hits (the hand-over is synchronisation latency: 12 -> 7 per step).
// The hit records are separate from what the apply kernel wrote back (dpz / dE) and from the host's copy of the permutation.
static int temp_hits_sync(amc_ctx *c, int case_id)
{
    amc_temp_ws &T = c->T;
    if (case_id <= 9) {
        AMC_HIP(c, amc_launch_temp_hits(c, case_id));
        AMC_HIP(c, hipMemcpyAsync(T.h_count, T.count, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    }
    AMC_HIP(c, hipStreamSynchronize(c->stream));    // the records are in host memory now (the kernel wrote them there)
    return AMC_OK;
}

int amc_wall_hits(amc_ctx *c, int case_id, int32_t *idx, double *normal_xyz, double *contact_z, size_t cap, size_t *n)
{
    if (!c || !n || case_id < 3 || case_id > 9) return AMC_ERR_INVALID;
    AMC_HIP(c, hipSetDevice(c->device));
    int rc = temp_ensure(c);
    if (rc) return rc;
    amc_temp_ws &T = c->T;
    amc_temp_handover &H = T.h;
    const bool ahead = H.ahead_case == case_id;     // launched behind the previous case's apply kernel, synchronised with it
    H.ahead_case = -1;
    if (!ahead && (rc = temp_hits_sync(c, case_id))) return rc;
    const int cnt = *T.h_count;
    if (cnt > T.cap) return amc_fail(c, AMC_ERR_CAPACITY, "%d wall hits exceed the record capacity %d", cnt, T.cap);
    if ((size_t)cnt > cap) return amc_fail(c, AMC_ERR_CAPACITY, "%d wall hits, caller buffer holds %zu", cnt, cap);
    H.hits_case = case_id; H.hits_n = cnt;
    temp_order(T.h_idx, (size_t)cnt, H.perm);
    *n = (size_t)cnt;
    for (int s = 0; s < cnt; s++) {
        const int k = H.perm[s];
        if (idx) idx[s] = T.h_idx[k];
        for (int e = 0; e < 3 && normal_xyz; e++) normal_xyz[3 * s + e] = T.h_normal[3 * k + e];
        if (contact_z) contact_z[s] = T.h_contact[3 * k + 2];
    }
    return AMC_OK;
}

// amc_wall_apply / amc_wall_park: the call matches the pending amc_wall_hits, else AMC_ERR_STATE
static int temp_match_hits(amc_ctx *c, const char *who, int case_id, size_t n)
{
    const amc_temp_handover &H = c->T.h;
    if (c->T.idx && H.hits_case == case_id && (size_t)H.hits_n == n) return AMC_OK;
    return amc_fail(c, AMC_ERR_STATE, "%s(case %d, n=%zu) does not match the pending amc_wall_hits(case %d, n=%d)", who, case_id, n, H.hits_case, H.hits_n);
}

// caller order (ascending particle index) -> record order, written where the kernel reads it (no energies yet: zeros)
static void temp_scatter(amc_temp_ws &T, const double *dir_xyz, const double *surface_energy, size_t n)
{
    for (size_t s = 0; s < n; s++) {
        const int k = T.h.perm[s];
        for (int e = 0; e < 3; e++) T.h_dir[3 * k + e] = dir_xyz[3 * s + e];
        T.h_Es[k] = surface_energy ? surface_energy[s] : 0.0;
    }
}

// record order -> caller order: what a kernel wrote back for the n hits behind `perm`
static void temp_gather(const std::vector<int> &perm, size_t n, const double *h_dpz, const double *h_dE, double *dpz, double *dE)
{
    for (size_t s = 0; s < n; s++) {
        if (dpz) dpz[s] = h_dpz[perm[s]];
        if (dE) dE[s] = h_dE[perm[s]];
    }
}

int amc_wall_apply(amc_ctx *c, int case_id, const double *dir_xyz, const double *surface_energy, size_t n, double *dpz, double *dE)
{
    if (!c) return AMC_ERR_INVALID;
    AMC_HIP(c, hipSetDevice(c->device));
    amc_temp_ws &T = c->T;
    int rc = temp_match_hits(c, "amc_wall_apply", case_id, n);
    if (rc) return rc;
    T.h.hits_case = -1;
    if (n == 0) return AMC_OK;
    if (!dir_xyz || !surface_energy) return AMC_ERR_INVALID;
    temp_scatter(T, dir_xyz, surface_energy, n);
    AMC_HIP(c, amc_launch_temp_apply(c, case_id, (int)n));
    if (c->SF.on) AMC_HIP(c, amc_launch_surface_case(c, case_id, (int)n));      // (in front of the next case's hits: they reuse the records)
    if ((rc = temp_hits_sync(c, case_id + 1))) return rc;
    T.h.ahead_case = case_id < 9 ? case_id + 1 : -1;
    temp_gather(T.h.perm, n, T.h_dpz, T.h_dE, dpz, dE);
    return AMC_OK;
}

// A case whose surface energies are not there yet (the gap case: mpmath integrals in worker processes, energised.py) can be
// PARKED: amc_wall_park does everything of amc_wall_apply that does not depend on the energy — the completed path, the
// counters, the particle at its contact point — so that the following cases' masks see what they have to see, and
// amc_wall_finish sets the new velocities when the energies have arrived.  Exact as long as no later case hits a parked
// particle before the finish (the driver checks the hit lists and finishes first if one does; amc_wall_hits_again makes
// the library evaluate that case's hits anew, on the finished state).
int amc_wall_park(amc_ctx *c, int case_id, const double *dir_xyz, size_t n)
{
    if (!c) return AMC_ERR_INVALID;
    AMC_HIP(c, hipSetDevice(c->device));
    amc_temp_ws &T = c->T;
    amc_temp_handover &H = T.h;
    int rc = temp_match_hits(c, "amc_wall_park", case_id, n);
    if (rc) return rc;
    if (H.parked_case >= 0) return amc_fail(c, AMC_ERR_STATE, "amc_wall_park: case %d is still parked", H.parked_case);
    H.hits_case = -1;
    H.parked_case = case_id; H.parked_n = 0;    // (a shard without a hit of its own parks nothing and finishes nothing)
    if (n == 0) return AMC_OK;
    if (!dir_xyz) return AMC_ERR_INVALID;
    temp_scatter(T, dir_xyz, nullptr, n);
    AMC_HIP(c, amc_launch_temp_apply(c, case_id, (int)n, true));
    if (c->SF.on && (rc = amc_surface_park(c, case_id, (int)n))) return rc;     // (the contact points do not outlive the next case's hits)
    H.parked_n = (int)n; H.parked_perm = H.perm;
    if ((rc = temp_hits_sync(c, case_id + 1))) return rc;
    H.ahead_case = case_id < 9 ? case_id + 1 : -1;
    return AMC_OK;
}

int amc_wall_finish(amc_ctx *c, int case_id, const double *surface_energy, size_t n, double *dpz, double *dE)
{
    if (!c) return AMC_ERR_INVALID;
    AMC_HIP(c, hipSetDevice(c->device));
    amc_temp_ws &T = c->T;
    amc_temp_handover &H = T.h;
    if (H.parked_case != case_id || (size_t)H.parked_n != n)
        return amc_fail(c, AMC_ERR_STATE, "amc_wall_finish(case %d, n=%zu) does not match the parked case %d (n=%d)", case_id, n, H.parked_case, H.parked_n);
    H.parked_case = -1;
    if (n == 0) return AMC_OK;
    if (!surface_energy) return AMC_ERR_INVALID;
    for (size_t s = 0; s < n; s++) T.h_def_Es[H.parked_perm[s]] = surface_energy[s];
    AMC_HIP(c, amc_launch_temp_velocity(c, case_id, (int)n));
    if (c->SF.on) AMC_HIP(c, amc_launch_surface_finish(c, case_id, (int)n));
    AMC_HIP(c, hipStreamSynchronize(c->stream));
    temp_gather(H.parked_perm, n, T.h_def_dpz, T.h_def_dE, dpz, dE);
    return AMC_OK;
}

int amc_wall_hits_again(amc_ctx *c)
{
    if (!c) return AMC_ERR_INVALID;
    c->T.h.ahead_case = -1;         // the hits launched behind the last apply are not used: the next amc_wall_hits evaluates its case anew
    c->T.h.hits_case = -1;
    return AMC_OK;
}

// ---- device-RNG mode ---------------------------------------------------------------------------------------------------------
static int temp_dev_ensure(amc_ctx *c)
{
    if (c->P.geometry != AMC_GEOM_PORE_ENERGISED) return amc_fail(c, AMC_ERR_STATE, "energised-wall calls need AMC_GEOM_PORE_ENERGISED");
    if (c->TD.seg.idx) return AMC_OK;
    amc_alloc_group group(c);
    int icap = (int)std::min<int64_t>(std::max<int64_t>(4096, c->n / 64 + 1024), 0x0fffffff);
    // AMC_TEMP_DEV_CAP (diagnostic): fewer records per case, so that a test reaches the overflow path with a handful of hits
    if (const char *e = getenv("AMC_TEMP_DEV_CAP")) { const int v = atoi(e); if (v > 0 && v < icap) icap = v; }
    const size_t cap = (size_t)icap * 7;
    temp_dev_segments D;
    D.cap = icap;
    AMC_HIP(c, dalloc(c, &D.idx, cap)); AMC_HIP(c, dalloc(c, &D.count, 8)); AMC_HIP(c, dalloc(c, &D.t, cap));
    AMC_HIP(c, dalloc(c, &D.contact, 3 * cap)); AMC_HIP(c, dalloc(c, &D.normal, 3 * cap)); AMC_HIP(c, dalloc(c, &D.dir, 3 * cap));
    AMC_HIP(c, dalloc(c, &D.Es, cap)); AMC_HIP(c, dalloc(c, &D.dpz, cap)); AMC_HIP(c, dalloc(c, &D.dE, cap)); AMC_HIP(c, dalloc(c, &D.ok, cap));
    group.keep();
    c->TD.seg = D;              // (published whole: seg.idx is the guard)
    return AMC_OK;
}

static int temp_rng_check(amc_ctx *c, const amc_temp_rng *cfg)
{
    if (cfg && cfg->struct_size == (int32_t)sizeof(amc_temp_rng) && cfg->n_gl >= 2 && cfg->n_gl <= 32) return AMC_OK;
    return amc_fail(c, AMC_ERR_INVALID, "amc_temp_rng: bad struct_size / n_gl");
}

// ---- the wall law of the device-RNG steps (include/argonmc-walllaw.h): host state, read by the launches -----------------------
int amc_temp_wall_law(amc_ctx *c, const amc_wall_law *law)
{
    if (!c) return AMC_ERR_INVALID;
    if (c->P.geometry != AMC_GEOM_PORE_ENERGISED) return amc_fail(c, AMC_ERR_STATE, "amc_temp_wall_law needs AMC_GEOM_PORE_ENERGISED");
    if (!law) { c->wall_law = amc_wall_law{}; return AMC_OK; }
    if (law->struct_size != (int32_t)sizeof(amc_wall_law)) return amc_fail(c, AMC_ERR_INVALID, "amc_wall_law: bad struct_size");
    if (law->kind != AMC_WALL_LAW_REFERENCE && law->kind != AMC_WALL_LAW_MAXWELL)
        return amc_fail(c, AMC_ERR_INVALID, "amc_wall_law: unknown kind %d", (int)law->kind);
    if (!(law->alpha_coated >= 0.0 && law->alpha_coated <= 1.0) || !(law->alpha_gap >= 0.0 && law->alpha_gap <= 1.0))
        return amc_fail(c, AMC_ERR_INVALID, "amc_wall_law: alpha_coated %g / alpha_gap %g outside [0, 1]", law->alpha_coated, law->alpha_gap);
    for (int k = 0; k < 4; k++)
        if (!(law->reserved[k] == 0.0)) return amc_fail(c, AMC_ERR_INVALID, "amc_wall_law: reserved words must be 0");
    c->wall_law = *law;
    return AMC_OK;
}

int amc_temp_wall_law_get(amc_ctx *c, amc_wall_law *out)
{
    if (!c || !out) return AMC_ERR_INVALID;
    if (c->P.geometry != AMC_GEOM_PORE_ENERGISED) return amc_fail(c, AMC_ERR_STATE, "amc_temp_wall_law_get needs AMC_GEOM_PORE_ENERGISED");
    if (c->wall_law.struct_size) { *out = c->wall_law; return AMC_OK; }
    *out = amc_wall_law{};
    out->struct_size = (int32_t)sizeof(amc_wall_law);
    out->kind = AMC_WALL_LAW_REFERENCE;
    out->alpha_coated = c->P.alpha_coated; out->alpha_gap = c->P.alpha_gap;
    return AMC_OK;
}

int amc_temp_cases_device(amc_ctx *c, const amc_temp_rng *cfg)
{
    if (!c || !c->uploaded) return AMC_ERR_STATE;
    int rc = temp_rng_check(c, cfg);
    if (rc) return rc;
    AMC_HIP(c, hipSetDevice(c->device));
    if ((rc = temp_dev_ensure(c))) return rc;
    if (!c->keep_prior) return amc_fail(c, AMC_ERR_STATE, "amc_temp_cases_device follows amc_temp_begin");
    c->TD.fetched = false;
    AMC_HIP(c, amc_launch_temp_cases_device(c, cfg));
    if (c->SF.on) AMC_HIP(c, amc_launch_surface_device(c));
    c->MG.step.hits = AMC_MG_HITS_LAUNCHED;     // (a sharded step's hits exchange may follow: amc_mg_hits_pack)
    return AMC_OK;
}

// the first k records' particle and results of segment s -> the host copies, queued on `st`
static int temp_dev_get(amc_ctx *c, amc_stage &st, int s, size_t k)
{
    amc_temp_dev_ws &D = c->TD;
    const size_t o = (size_t)s * (size_t)D.seg.cap;
    D.h_idx[s].resize(k); D.h_dpz[s].resize(k); D.h_dE[s].resize(k); D.h_ok[s].resize(k);
    AMC_HIP(c, st.get(D.h_idx[s].data(), D.seg.idx + o, sizeof(int) * k));
    AMC_HIP(c, st.get(D.h_dpz[s].data(), D.seg.dpz + o, sizeof(double) * k));
    AMC_HIP(c, st.get(D.h_dE[s].data(), D.seg.dE + o, sizeof(double) * k));
    AMC_HIP(c, st.get(D.h_ok[s].data(), D.seg.ok + o, k));
    return AMC_OK;
}

// counts of all seven cases and the head of every segment in one synchronisation; longer segments are completed here
static int temp_dev_fetch(amc_ctx *c)
{
    amc_temp_dev_ws &D = c->TD;
    if (D.fetched) return AMC_OK;
    const int cap = D.seg.cap, pre = std::min(cap, 2048);
    int rc;
    amc_stage st(c);
    AMC_HIP(c, st.get(D.h_count, D.seg.count, sizeof(int) * 7));
    for (int s = 0; s < 7; s++)
        if ((rc = temp_dev_get(c, st, s, (size_t)pre))) return rc;
    AMC_HIP(c, st.finish());
    for (int s = 0; s < 7; s++) {
        if (D.h_count[s] > cap) return amc_fail(c, AMC_ERR_CAPACITY, "%d wall hits in case %d exceed the record capacity %d", D.h_count[s], 3 + s, cap);
        const size_t k = (size_t)std::max(D.h_count[s], 0);
        if ((int)k > pre) {
            if ((rc = temp_dev_get(c, st, s, k))) return rc;
            AMC_HIP(c, st.finish());
        }
    }
    D.fetched = true;
    return AMC_OK;
}

int amc_temp_device_results(amc_ctx *c, int case_id, int32_t *idx, double *dpz, double *dE, uint8_t *ok, size_t cap, size_t *n)
{
    if (!c || !n || case_id < 3 || case_id > 9 || !c->TD.seg.idx) return AMC_ERR_INVALID;
    AMC_HIP(c, hipSetDevice(c->device));
    int rc = temp_dev_fetch(c);
    if (rc) return rc;
    amc_temp_dev_ws &D = c->TD;
    const int s = case_id - 3;
    const size_t k = (size_t)std::max(D.h_count[s], 0);
    if (k > cap) return amc_fail(c, AMC_ERR_CAPACITY, "%zu wall hits, caller buffer holds %zu", k, cap);
    std::vector<int> perm;
    temp_order(D.h_idx[s].data(), k, perm);
    for (size_t u = 0; u < k; u++) {
        const int r = perm[u];
        if (idx) idx[u] = D.h_idx[s][r];
        if (dpz) dpz[u] = D.h_dpz[s][r];
        if (dE) dE[u] = D.h_dE[s][r];
        if (ok) ok[u] = D.h_ok[s][r];
    }
    *n = k;
    return AMC_OK;
}

int amc_temp_device_sums(amc_ctx *c, double *sums, int32_t *had)
{
    if (!c || !sums || !had || !c->TD.seg.idx) return AMC_ERR_INVALID;
    AMC_HIP(c, hipSetDevice(c->device));
    int rc = temp_dev_fetch(c);
    if (rc) return rc;
    amc_temp_dev_ws &D = c->TD;
    // k_case_sums's order (amc_case_sums_dev.h) on the host's copies of the records
    double m[7], e[7];
    int any[7], present[7];
    std::vector<int> perm;
    for (int s = 0; s < 7; s++) {
        const size_t k = (size_t)amc_clamp_count(D.h_count[s], D.seg.cap);
        m[s] = e[s] = 0.0; any[s] = 0; present[s] = k != 0;
        temp_order(D.h_idx[s].data(), k, perm);
        for (size_t u = 0; u < k; u++) {
            const int r = perm[u];
            if (D.h_ok[s][r]) { m[s] = m[s] + D.h_dpz[s][r]; e[s] = e[s] + D.h_dE[s][r]; any[s] = 1; }
        }
    }
    const amc_temp_row row = amc_fold_cases(m, e, any, present);
    for (int k = 0; k < 3; k++) { sums[k] = row.sums[k]; had[k] = (row.had >> k) & 1; }
    return AMC_OK;
}

int amc_temp_device_draws(amc_ctx *c, int case_id, int32_t *idx, double *normal_xyz, double *contact_z, double *dir_xyz,
                          double *surface_energy, size_t cap, size_t *n)
{
    if (!c || !n || case_id < 3 || case_id > 9 || !c->TD.seg.idx) return AMC_ERR_INVALID;
    AMC_HIP(c, hipSetDevice(c->device));
    int rc = temp_dev_fetch(c);
    if (rc) return rc;
    amc_temp_dev_ws &D = c->TD;
    const int s = case_id - 3;
    const size_t k = (size_t)std::max(D.h_count[s], 0), o = (size_t)s * (size_t)D.seg.cap;
    if (k > cap) return amc_fail(c, AMC_ERR_CAPACITY, "%zu wall hits, caller buffer holds %zu", k, cap);
    *n = k;
    if (!k) return AMC_OK;
    std::vector<double> hn(3 * k), hc(3 * k), hd(3 * k), he(k);
    AMC_HIP(c, hipMemcpy(hn.data(), D.seg.normal + 3 * o, sizeof(double) * 3 * k, hipMemcpyDeviceToHost));
    AMC_HIP(c, hipMemcpy(hc.data(), D.seg.contact + 3 * o, sizeof(double) * 3 * k, hipMemcpyDeviceToHost));
    AMC_HIP(c, hipMemcpy(hd.data(), D.seg.dir + 3 * o, sizeof(double) * 3 * k, hipMemcpyDeviceToHost));
    AMC_HIP(c, hipMemcpy(he.data(), D.seg.Es + o, sizeof(double) * k, hipMemcpyDeviceToHost));
    std::vector<int> perm;
    temp_order(D.h_idx[s].data(), k, perm);
    for (size_t u = 0; u < k; u++) {
        const int r = perm[u];
        if (idx) idx[u] = D.h_idx[s][r];
        for (int e = 0; e < 3; e++) {
            if (normal_xyz) normal_xyz[3 * u + e] = hn[3 * r + e];
            if (dir_xyz) dir_xyz[3 * u + e] = hd[3 * r + e];
        }
        if (contact_z) contact_z[u] = hc[3 * r + 2];
        if (surface_energy) surface_energy[u] = he[r];
    }
    return AMC_OK;
}

// contact points of the last device-RNG step's hits of a case, ascending particle index (sampled surfaces: inspection)
int amc_temp_device_contacts(amc_ctx *c, int case_id, int32_t *idx, double *contact_xyz, size_t cap, size_t *n)
{
    if (!c || !n || case_id < 3 || case_id > 9 || !c->TD.seg.idx) return AMC_ERR_INVALID;
    AMC_HIP(c, hipSetDevice(c->device));
    int rc = temp_dev_fetch(c);
    if (rc) return rc;
    amc_temp_dev_ws &D = c->TD;
    const int s = case_id - 3;
    const size_t k = (size_t)std::max(D.h_count[s], 0), o = (size_t)s * (size_t)D.seg.cap;
    if (k > cap) return amc_fail(c, AMC_ERR_CAPACITY, "%zu wall hits, caller buffer holds %zu", k, cap);
    *n = k;
    if (!k) return AMC_OK;
    std::vector<double> hc(3 * k);
    AMC_HIP(c, hipMemcpy(hc.data(), D.seg.contact + 3 * o, sizeof(double) * 3 * k, hipMemcpyDeviceToHost));
    std::vector<int> perm;
    temp_order(D.h_idx[s].data(), k, perm);
    for (size_t u = 0; u < k; u++) {
        const int r = perm[u];
        if (idx) idx[u] = D.h_idx[s][r];
        for (int e = 0; e < 3 && contact_xyz; e++) contact_xyz[3 * u + e] = hc[3 * r + e];
    }
    return AMC_OK;
}

// ... and of the pending amc_wall_hits, in its order
int amc_wall_contacts(amc_ctx *c, int case_id, double *contact_xyz, size_t cap)
{
    if (!c || !contact_xyz) return AMC_ERR_INVALID;
    const amc_temp_ws &T = c->T;
    const amc_temp_handover &H = T.h;
    if (!T.idx || H.hits_case != case_id)
        return amc_fail(c, AMC_ERR_STATE, "amc_wall_contacts(case %d): the pending amc_wall_hits is of case %d", case_id, H.hits_case);
    if ((size_t)H.hits_n > cap) return amc_fail(c, AMC_ERR_CAPACITY, "%d wall hits, caller buffer holds %zu", H.hits_n, cap);
    for (int s = 0; s < H.hits_n; s++)
        for (int e = 0; e < 3; e++) contact_xyz[3 * s + e] = T.h_contact[3 * H.perm[s] + e];
    return AMC_OK;
}

// ---- the host-free run of the device-RNG mode ------------------------------------------------------------------------------
// the series buffer for `rows` steps, the ordering scratch and the overflow words of the sums kernel, the pass's constants
static int temp_run_ensure(amc_ctx *c, int64_t rows)
{
    amc_temp_dev_ws &D = c->TD;
    if (!D.ovf) {
        amc_alloc_group group(c);
        int *perm, *ovf;
        amc_temp_pass *pass;
        AMC_HIP(c, dalloc(c, &perm, (size_t)7 * (size_t)D.seg.cap));
        AMC_HIP(c, dalloc(c, &pass, 1));
        AMC_HIP(c, dalloc(c, &ovf, 4));
        group.keep();
        D.perm = perm; D.pass = pass;
        D.ovf = ovf;            // (the guard: last)
    }
    if (rows > D.series_cap) {
        amc_temp_row *series;
        AMC_HIP(c, dalloc(c, &series, (size_t)rows));
        AMC_HIP(c, hipStreamSynchronize(c->stream));        // (nothing in flight writes the old rows)
        ctx_free(c, D.series);
        D.series = series; D.series_cap = rows;
    }
    return AMC_OK;
}

int amc_temp_run_device(amc_ctx *c, double dt, int64_t nsteps, const amc_temp_rng *cfg, amc_step_stats *sum)
{
    if (!c) return AMC_ERR_INVALID;
    if (c->P.geometry != AMC_GEOM_PORE_ENERGISED) return amc_fail(c, AMC_ERR_STATE, "amc_temp_run_device needs AMC_GEOM_PORE_ENERGISED");
    int rc = temp_rng_check(c, cfg);
    if (rc) return rc;
    if (nsteps < 0 || nsteps > 0x3fffffffLL) return amc_fail(c, AMC_ERR_INVALID, "amc_temp_run_device: nsteps %lld out of range", (long long)nsteps);
    if (!c->uploaded) return amc_fail(c, AMC_ERR_STATE, "amc_temp_run_device before amc_upload");
    if (c->lo != 0 || c->hi != c->n) return amc_fail(c, AMC_ERR_STATE, "amc_temp_run_device needs the whole index range in one context");
    AMC_HIP(c, hipSetDevice(c->device));
    if ((rc = temp_dev_ensure(c))) return rc;
    if ((rc = temp_run_ensure(c, std::max<int64_t>(nsteps, 1)))) return rc;
    amc_temp_dev_ws &D = c->TD;
    if ((rc = amc_flush(c))) return rc;
    D.series_n = 0;
    D.fetched = false;
    c->T.h.fresh();
    amc_mg_step_fresh(c);
    c->keep_prior = true;               // (as after amc_temp_begin)
    AMC_HIP(c, hipMemsetAsync(D.ovf, 0, 4 * sizeof(int), c->stream));
    const bool fuse = !c->allpairs;     // the detection grid's lists are filed by the last pass in front of the sweep
    const bool fused = !c->temp_run_unfused;
    if (fused && nsteps > 0) {
        amc_temp_pass h;
        memset(&h, 0, sizeof h);
        h.g = *cfg; h.D = D.seg;
        AMC_HIP(c, hipMemcpyAsync(D.pass, &h, sizeof h, hipMemcpyHostToDevice, c->stream));
        AMC_HIP(c, hipStreamSynchronize(c->stream));        // (the source is this frame's)
    }
    bool deferred = false;              // the previous step left its post-sweep recapture (Temp:844) to this step's pass
    for (int64_t s = 0; s < nsteps; s++) {
        if (fused) {
            // ONE pass in front of the sweep: drift, cases 1-2, cases 3-9 with the device draws, recapture (Temp:804), filing
            AMC_HIP(c, hipMemsetAsync(D.seg.count, 0, sizeof(int) * 7, c->stream));
            AMC_HIP(c, amc_launch_stream(c, dt, AMC_ST_DRIFT | AMC_ST_WALLS | AMC_ST_TEMP_CASES | AMC_ST_BOUNDS | (deferred ? AMC_ST_BOUNDS_PRE : 0),
                                         0, fuse));
        } else {
            // what amc_temp_begin, amc_temp_cases_device and amc_temp_end enqueue
            AMC_HIP(c, amc_launch_stream(c, dt, AMC_ST_DRIFT | AMC_ST_WALLS, 0));
            AMC_HIP(c, amc_launch_temp_cases_device(c, cfg));
            AMC_HIP(c, amc_launch_stream(c, 0.0, AMC_ST_BOUNDS, 0, fuse));
        }
        AMC_HIP(c, amc_launch_temp_sums(c, s));
        if (c->SF.on) AMC_HIP(c, amc_launch_surface_device(c));     // (in front of the next step's pass, which clears seg.count)
        if ((rc = amc_enqueue_sweep(c, fuse))) return rc;                               // Temp:813-842
        // a sampled step and the last one end with the state everybody reads: their recapture is a pass of its own
        deferred = fused && s + 1 < nsteps && !amc_samplers_due(c, (int64_t)c->out.step + 1);
        if (!deferred) AMC_HIP(c, amc_launch_stream(c, 0.0, AMC_ST_BOUNDS, 1));       // Temp:844
        c->out.step++;
        if (c->SF.on) c->SF.n_steps++;
        if ((rc = amc_samplers_step(c))) return rc;
    }
    D.series_n = nsteps;
    rc = amc_finish_stats(c, sum);      // the one synchronisation; overflow flags and counters of the whole run
    int ovf[4] = {0, 0, 0, 0};
    AMC_HIP(c, hipMemcpy(ovf, D.ovf, sizeof ovf, hipMemcpyDeviceToHost));
    if (ovf[0] || rc == AMC_ERR_CAPACITY) c->SF.lost = c->SF.on;     // hits are missing from the sampled surfaces
    if (ovf[0] || rc == AMC_ERR_CAPACITY) c->MF.lost = c->MF.on;     // ... and paths from the sampled free paths
    if (ovf[0]) {
        D.series_n = 0;
        return amc_fail(c, AMC_ERR_CAPACITY, "%d wall hits in case %d exceed the record capacity %d (step %d of the run)", ovf[2], ovf[0], D.seg.cap, ovf[1]);
    }
    if (rc) D.series_n = 0;
    return rc;
}

// ---- the host-free run over shards: the steps themselves are the amc_temp_* / amc_mg_* calls ------------------
int amc_temp_shard_run_begin(amc_ctx *c, int64_t nsteps)
{
    if (!c) return AMC_ERR_INVALID;
    if (c->P.geometry != AMC_GEOM_PORE_ENERGISED) return amc_fail(c, AMC_ERR_STATE, "amc_temp_shard_run_begin needs AMC_GEOM_PORE_ENERGISED");
    if (nsteps < 0 || nsteps > 0x3fffffffLL) return amc_fail(c, AMC_ERR_INVALID, "amc_temp_shard_run_begin: nsteps %lld out of range", (long long)nsteps);
    if (!c->uploaded) return amc_fail(c, AMC_ERR_STATE, "amc_temp_shard_run_begin before amc_upload");
    if (int rc = amc_mg_step_idle(c, "amc_temp_shard_run_begin")) return rc;
    AMC_HIP(c, hipSetDevice(c->device));
    int rc;
    if ((rc = temp_dev_ensure(c))) return rc;
    if ((rc = temp_run_ensure(c, std::max<int64_t>(nsteps, 1)))) return rc;
    amc_temp_dev_ws &D = c->TD;
    D.series_n = 0;
    D.fetched = false;
    c->MG.hits_rows = nsteps;
    AMC_HIP(c, hipMemsetAsync(D.ovf, 0, 4 * sizeof(int), c->stream));
    return AMC_OK;
}

int amc_temp_shard_run_end(amc_ctx *c, int64_t nsteps, amc_step_stats *sum)
{
    if (!c) return AMC_ERR_INVALID;
    amc_temp_dev_ws &D = c->TD;
    if (!D.ovf || nsteps < 0 || nsteps > c->MG.hits_rows)
        return amc_fail(c, AMC_ERR_STATE, "amc_temp_shard_run_end(%lld steps) does not match amc_temp_shard_run_begin(%lld)", (long long)nsteps, (long long)c->MG.hits_rows);
    AMC_HIP(c, hipSetDevice(c->device));
    c->MG.hits_rows = 0;
    D.series_n = nsteps;
    int rc = amc_finish_stats(c, sum);  // the one synchronisation; overflow flags and counters of the whole run
    int ovf[4] = {0, 0, 0, 0};
    AMC_HIP(c, hipMemcpy(ovf, D.ovf, sizeof ovf, hipMemcpyDeviceToHost));
    if (ovf[0] || ovf[3] || rc == AMC_ERR_CAPACITY) c->SF.lost = c->SF.on;      // hits are missing from the sampled surfaces
    if (ovf[0] || ovf[3] || rc == AMC_ERR_CAPACITY) c->MF.lost = c->MF.on;      // ... and paths from the sampled free paths
    if (ovf[0]) {
        D.series_n = 0;
        if (ovf[2] == 0x7fffffff)
            return amc_fail(c, AMC_ERR_CAPACITY, "the wall hits of one rank in case %d exceed its record capacity %d (step %d of the run)", ovf[0], D.seg.cap, ovf[1]);
        return amc_fail(c, AMC_ERR_CAPACITY, "%d wall hits of one rank in case %d exceed the hits exchange's capacity %d (step %d of the run)", ovf[2], ovf[0],
                        c->MG.hits_cap, ovf[1]);
    }
    if (ovf[3] && !rc) {                // (flagged by this rank's pack alone: no sums call followed it)
        D.series_n = 0;
        return amc_fail(c, AMC_ERR_CAPACITY, "wall hits of this rank exceed the hits exchange's capacity %d", c->MG.hits_cap);
    }
    if (rc) D.series_n = 0;
    return rc;
}

int amc_temp_series_read(amc_ctx *c, int64_t first, int64_t count, double *sums, uint8_t *had, int64_t *n_steps)
{
    if (!c) return AMC_ERR_INVALID;
    const amc_temp_dev_ws &D = c->TD;
    if (n_steps) *n_steps = D.series_n;
    if (first < 0 || count < 0 || first + count > D.series_n)
        return amc_fail(c, AMC_ERR_INVALID, "amc_temp_series_read: rows %lld .. %lld of a run of %lld steps", (long long)first,
                        (long long)(first + count) - 1, (long long)D.series_n);
    if (!count) return AMC_OK;
    AMC_HIP(c, hipSetDevice(c->device));
    std::vector<amc_temp_row> rows((size_t)count);
    AMC_HIP(c, hipMemcpyAsync(rows.data(), D.series + first, sizeof(amc_temp_row) * (size_t)count, hipMemcpyDeviceToHost, c->stream));
    AMC_HIP(c, hipStreamSynchronize(c->stream));
    for (int64_t k = 0; k < count; k++)
        for (int e = 0; e < 3; e++) {
            if (sums) sums[3 * k + e] = rows[(size_t)k].sums[e];
            if (had) had[3 * k + e] = (rows[(size_t)k].had >> e) & 1u;
        }
    return AMC_OK;
}

int amc_set_step(amc_ctx *c, int64_t step)
{
    if (!c) return AMC_ERR_INVALID;
    if (step < 0 || step > 0x3fffffffLL) return amc_fail(c, AMC_ERR_INVALID, "amc_set_step: step %lld out of range", (long long)step);
    c->out.step = (int)step;
    return AMC_OK;
}

int amc_temp_end(amc_ctx *c, amc_step_stats *out)
{
    if (!c || !c->uploaded) return AMC_ERR_STATE;
    AMC_HIP(c, hipSetDevice(c->device));
    if (c->P.geometry != AMC_GEOM_PORE_ENERGISED) return amc_fail(c, AMC_ERR_STATE, "amc_temp_end needs AMC_GEOM_PORE_ENERGISED");
    if (c->T.h.parked_case >= 0) return amc_fail(c, AMC_ERR_STATE, "amc_temp_end: case %d is still parked", c->T.h.parked_case);
    c->T.h.ahead_case = -1;
    // the bounds pass before the sweep sees every particle at its final pre-sweep position: it builds the detection
    // grid's lists as well (like the fused streaming pass of the specular geometries)
    const bool fuse = !c->allpairs && c->lo == 0 && c->hi == c->n;
    AMC_HIP(c, amc_launch_stream(c, 0.0, AMC_ST_BOUNDS, 0, fuse));  // Temp:804
    int rc = amc_enqueue_sweep(c, fuse);                                // Temp:813-842
    if (rc) return rc;
    AMC_HIP(c, amc_launch_stream(c, 0.0, AMC_ST_BOUNDS, 1));        // Temp:844
    c->out.step++;
    if (c->SF.on) c->SF.n_steps++;
    if ((rc = amc_samplers_step(c))) return rc;
    rc = amc_finish_stats(c, out);
    if (rc == AMC_ERR_CAPACITY) c->SF.lost = c->SF.on;              // hits are missing from the sampled surfaces
    if (rc == AMC_ERR_CAPACITY) c->MF.lost = c->MF.on;              // ... and paths from the sampled free paths
    return rc;
}

}  // extern "C"
