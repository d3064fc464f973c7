// amc_energised.hip — the deterministic part of Temperature_Pore_MC.py's energised wall handlers (Temp:349-553) on
// the GPU, split around the host-side random draws (Temp:119-141) and mpmath energies (Temp:143-152):
//
//   k_temp_hits   evaluates the mask of ONE case (Temp:708-751) on the current state, and for every hit computes the
//                 flight time since contact, the contact point and the inward unit normal (compacted records);
//   (host)        sorts the records by particle index, draws a direction per hit from the two Mersenne Twisters in that
//                 order, evaluates the surface energy;
//   k_temp_apply  energy accommodation, new velocity, free-path bookkeeping, particle parked at the contact point,
//                 per-hit z-momentum and energy changes (summed by the host in hit order, like Temp:385-389).
//
// The cases are sequential in the reference (each mask is evaluated after the previous handler ran), hence one
// hits/apply pair per case.  Both kernels are O(N) streaming passes over positions (+prior); hits are ~1e-3 of N.
#include "amc_energised_dev.h"

struct temp_records {
    int *idx;
    double *t, *contact, *normal;   // [cap], [3*cap], [3*cap]
    unsigned char *ok;
    int *count;
    int cap;
};


__global__ __launch_bounds__(256) void k_temp_hits(amc_state S, amc_params P, int case_id, long long lo, long long hi,
                                                   temp_records R, amc_dev_counters *cnt)
{
    const long long p = lo + (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= hi) return;
    const double x = S.x[p], y = S.y[p], z = S.z[p];
    if (!temp_mask(P, case_id, x, y, z, S.px[p], S.py[p], S.pz[p])) return;
    const int k = atomicAdd(R.count, 1);
    if (k >= R.cap) { atomicOr(&cnt->flags, 4ULL); return; }
    R.idx[k] = (int)p;
    const temp_contact c = temp_solve(P, case_id, x, y, z, S.vx[p], S.vy[p], S.vz[p]);
    R.t[k] = c.t; R.ok[k] = c.ok;
    R.contact[3 * k] = c.cx; R.contact[3 * k + 1] = c.cy; R.contact[3 * k + 2] = c.cz;
    R.normal[3 * k] = c.n0; R.normal[3 * k + 1] = c.n1; R.normal[3 * k + 2] = c.n2;
}

// `park` (the gap case with its surface energies still being integrated on the host, amc_wall_park): everything of the
// handler that does not depend on the energy — completed path (old velocity), counters, accumulators zeroed, particle at the
// contact point — and the hit's particle and direction kept in `def_idx` / `def_dir`; k_temp_velocity finishes it.
__global__ __launch_bounds__(256) void k_temp_apply(amc_state S, amc_params P, amc_out O, int case_id, int n,
                                                    temp_records R, const double *__restrict__ dir,
                                                    const double *__restrict__ Es, double *__restrict__ dpz,
                                                    double *__restrict__ dE, int park, int *__restrict__ def_idx,
                                                    double *__restrict__ def_dir)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (n < 0) n = min(*R.count, R.cap);        // device-RNG mode: the host never saw the count
    if (k >= n) return;
    dpz[k] = 0; dE[k] = 0;
    if (park) { def_idx[k] = R.ok[k] ? R.idx[k] : -1; def_dir[3 * k] = dir[3 * k]; def_dir[3 * k + 1] = dir[3 * k + 1]; def_dir[3 * k + 2] = dir[3 * k + 2]; }
    if (!R.ok[k]) { atomicAdd(&O.banks[amc_bank_id()].n_fp_errors, 1ULL); atomicAdd(&O.banks[amc_bank_id()].n_wall, 1ULL); return; }
    const int p = R.idx[k];
    const double t = R.t[k];
    const double vx = S.vx[p], vy = S.vy[p], vz = S.vz[p];
    double wvx = vx, wvy = vy, wvz = vz;
    const double v_magnitude = park ? sqrt(vx * vx + vy * vy + vz * vz)                       // Temp:377 (as in temp_accommodate)
                                    : temp_accommodate(P, case_id, vx, vy, vz, Es[k], dir[3 * k], dir[3 * k + 1], dir[3 * k + 2],
                                                       wvx, wvy, wvz, dpz[k], dE[k]);
    if (S.flag[p])                                                                           // Temp:391-395
        amc_emit(O, case_id + 1, 0, p, -1, 0, fabs(S.d[p] - fabs(v_magnitude * t)), fabs(S.dx[p] - fabs(vx * t)),
                 fabs(S.dy[p] - fabs(vy * t)), fabs(S.dz[p] - fabs(vz * t)));
    else
        S.flag[p] = 1;
    S.d[p] = 0; S.dx[p] = 0; S.dy[p] = 0; S.dz[p] = 0;                                       // Temp:398-401
    S.x[p] = R.contact[3 * k]; S.y[p] = R.contact[3 * k + 1]; S.z[p] = R.contact[3 * k + 2];   // Temp:402
    S.vx[p] = wvx; S.vy[p] = wvy; S.vz[p] = wvz;                                             // Temp:403
    atomicAdd(&O.banks[amc_bank_id()].n_wall, 1ULL);                                         // Temp:411,482,552
}

// the second half of a parked case: energy accommodation and the new velocity (Temp:377-388) from the velocity the particle
// still has (nothing touched it since it was parked) and the surface energies that have arrived
__global__ __launch_bounds__(256) void k_temp_velocity(amc_state S, amc_params P, int case_id, int n, const int *__restrict__ def_idx,
                                                       const double *__restrict__ def_dir, const double *__restrict__ Es,
                                                       double *__restrict__ dpz, double *__restrict__ dE)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    dpz[k] = 0; dE[k] = 0;
    const int p = def_idx[k];
    if (p < 0) return;                          // (a failed contact solve: counted when the case was parked)
    double wvx, wvy, wvz;
    temp_accommodate(P, case_id, S.vx[p], S.vy[p], S.vz[p], Es[k], def_dir[3 * k], def_dir[3 * k + 1], def_dir[3 * k + 2], wvx, wvy,
                     wvz, dpz[k], dE[k]);
    S.vx[p] = wvx; S.vy[p] = wvy; S.vz[p] = wvz;                                             // Temp:403
}

static temp_records make_records(amc_ctx *c)
{
    temp_records R;
    R.idx = c->T.idx; R.t = c->T.t; R.contact = c->T.contact; R.normal = c->T.normal; R.ok = c->T.ok;
    R.count = c->T.count; R.cap = c->T.cap;
    return R;
}

hipError_t amc_launch_temp_hits(amc_ctx *c, int case_id)
{
    const long long cnt = c->hi - c->lo;
    hipError_t e = hipMemsetAsync(c->T.count, 0, sizeof(int), c->stream);
    if (e != hipSuccess || cnt <= 0) return e;
    AMC_LAUNCH(c, k_temp_hits, dim3((unsigned)((cnt + 255) / 256)), dim3(256), c->S, c->P, case_id,
                       c->lo, c->hi, make_records(c), c->d_cnt);
    return hipGetLastError();
}

hipError_t amc_launch_temp_apply(amc_ctx *c, int case_id, int n, bool park)
{
    if (n <= 0) return hipSuccess;
    AMC_LAUNCH(c, k_temp_apply, dim3((n + 255) / 256), dim3(256), c->S, c->P, c->out, case_id, n,
                       make_records(c), c->T.dir, c->T.Es, c->T.dpz, c->T.dE, park ? 1 : 0, c->T.def_idx, c->T.def_dir);
    return hipGetLastError();
}

hipError_t amc_launch_temp_velocity(amc_ctx *c, int case_id, int n)
{
    if (n <= 0) return hipSuccess;
    AMC_LAUNCH(c, k_temp_velocity, dim3((n + 255) / 256), dim3(256), c->S, c->P, case_id, n, c->T.def_idx, c->T.def_dir,
               c->T.def_Es, c->T.def_dpz, c->T.def_dE);
    return hipGetLastError();
}


// ---- opt-in non-parity mode: directions and energies drawn on the device (include/argonmc.h, amc_temp_rng) -----------
__global__ __launch_bounds__(256) void k_temp_sample(amc_params P, amc_temp_rng g, int case_id, unsigned int step,
                                                     temp_records R, double *__restrict__ dir, double *__restrict__ Es)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= min(*R.count, R.cap)) return;
    dir[3 * k] = dir[3 * k + 1] = dir[3 * k + 2] = 0.0;
    Es[k] = 0.0;
    if (!R.ok[k]) return;
    double fx, fy, fz, e;
    temp_draw(P, g, case_id, step, R.idx[k], R.normal[3 * k], R.normal[3 * k + 1], R.normal[3 * k + 2], R.contact[3 * k + 2],
              fx, fy, fz, e);
    dir[3 * k] = fx; dir[3 * k + 1] = fy; dir[3 * k + 2] = fz;
    Es[k] = e;
}

// All seven energised cases of a step in ONE pass (device-RNG mode): every case reads and writes only the particle
// itself and the masks are evaluated in case order, each after the previous handler ran (Temp:705-758) — which per
// particle is a sequential evaluation (temp_cases_particle, amc_energised_dev.h), so with the random numbers available on
// the device the 7 x (hits, sample, apply) kernels collapse into this one.  The per-hit records (one segment per case) are
// still written: their z-momentum / energy changes are summed in the reference's order, tests read the draws.
// LAW (AMC_WALL_LAW_*): the context's wall law; the Maxwell instance gets the law's two alpha in P.alpha_coated / P.alpha_gap.
template <int LAW>
__global__ __launch_bounds__(256) void k_temp_all(amc_state S, amc_params P, amc_out O, amc_temp_rng g, unsigned int step,
                                                  long long lo, long long hi, temp_dev_segments D, amc_dev_counters *cnt)
{
    const long long p = lo + (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= hi) return;
    temp_particle q;
    q.x = S.x[p]; q.y = S.y[p]; q.z = S.z[p];
    const double px = S.px[p], py = S.py[p], pz = S.pz[p];
    if (!temp_any_mask(P, q.x, q.y, q.z, px, py, pz)) return;   // (a hit moves the particle: the masks are re-evaluated case by case)
    q.vx = S.vx[p]; q.vy = S.vy[p]; q.vz = S.vz[p];
    q.d = S.d[p]; q.dx = S.dx[p]; q.dy = S.dy[p]; q.dz = S.dz[p];
    q.flag = S.flag[p] != 0;
    temp_cases_particle<false, LAW>(P, O, g, step, D, (int)p, px, py, pz, q);
    S.x[p] = q.x; S.y[p] = q.y; S.z[p] = q.z; S.vx[p] = q.vx; S.vy[p] = q.vy; S.vz[p] = q.vz;
    S.d[p] = q.d; S.dx[p] = q.dx; S.dy[p] = q.dy; S.dz[p] = q.dz; S.flag[p] = q.flag ? 1 : 0;
    if (q.nwall) atomicAdd(&O.banks[amc_bank_id()].n_wall, (unsigned long long)q.nwall);
    if (q.nerr) atomicAdd(&O.banks[amc_bank_id()].n_fp_errors, (unsigned long long)q.nerr);
}

// The case-by-case form's draw and apply of one case under the Maxwell law (AMC_TEMP_UNFUSED=1): what k_temp_sample and
// k_temp_apply do under the reference law, in one kernel, because a specular reflection needs the incoming velocity where the
// reference's draw needs only the normal.  Same device functions, hence the same bits, as temp_cases_particle's Maxwell branch.
__global__ __launch_bounds__(256) void k_temp_maxwell(amc_state S, amc_params P, amc_out O, amc_temp_rng g, int case_id,
                                                      unsigned int step, temp_records R, double *__restrict__ dir,
                                                      double *__restrict__ Es, double *__restrict__ dpz, double *__restrict__ dE)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= min(*R.count, R.cap)) return;
    dir[3 * k] = dir[3 * k + 1] = dir[3 * k + 2] = 0.0;
    Es[k] = 0.0; dpz[k] = 0; dE[k] = 0;
    if (!R.ok[k]) { atomicAdd(&O.banks[amc_bank_id()].n_fp_errors, 1ULL); atomicAdd(&O.banks[amc_bank_id()].n_wall, 1ULL); return; }
    const int p = R.idx[k];
    const double t = R.t[k];
    const double vx = S.vx[p], vy = S.vy[p], vz = S.vz[p];
    double wvx, wvy, wvz, es, fx, fy, fz, mz, e;
    temp_maxwell_draw(P, g, case_id, step, p, R.normal[3 * k], R.normal[3 * k + 1], R.normal[3 * k + 2], R.contact[3 * k + 2], vx, vy, vz,
                      wvx, wvy, wvz, es);
    const double v_magnitude = temp_maxwell_finish(P, vx, vy, vz, wvx, wvy, wvz, fx, fy, fz, mz, e);
    dir[3 * k] = fx; dir[3 * k + 1] = fy; dir[3 * k + 2] = fz;
    Es[k] = es; dpz[k] = mz; dE[k] = e;
    if (S.flag[p])                                                                           // Temp:391-395
        amc_emit(O, case_id + 1, 0, p, -1, 0, fabs(S.d[p] - fabs(v_magnitude * t)), fabs(S.dx[p] - fabs(vx * t)),
                 fabs(S.dy[p] - fabs(vy * t)), fabs(S.dz[p] - fabs(vz * t)));
    else
        S.flag[p] = 1;
    S.d[p] = 0; S.dx[p] = 0; S.dy[p] = 0; S.dz[p] = 0;                                       // Temp:398-401
    S.x[p] = R.contact[3 * k]; S.y[p] = R.contact[3 * k + 1]; S.z[p] = R.contact[3 * k + 2];   // Temp:402
    S.vx[p] = wvx; S.vy[p] = wvy; S.vz[p] = wvz;                                             // Temp:403
    atomicAdd(&O.banks[amc_bank_id()].n_wall, 1ULL);                                         // Temp:411,482,552
}

// the context's parameters as the Maxwell instances take them: the law's alpha in place of the accommodation coefficients
amc_params amc_wall_law_params(const amc_ctx *c)
{
    amc_params P = c->P;
    if (amc_wall_law_kind(c) == AMC_WALL_LAW_MAXWELL) { P.alpha_coated = c->wall_law.alpha_coated; P.alpha_gap = c->wall_law.alpha_gap; }
    return P;
}

hipError_t amc_launch_temp_cases_device(amc_ctx *c, const amc_temp_rng *cfg)
{
    const bool maxwell = amc_wall_law_kind(c) == AMC_WALL_LAW_MAXWELL;
    const long long cnt = c->hi - c->lo;
    const temp_dev_segments &D = c->TD.seg;
    hipError_t e = hipMemsetAsync(D.count, 0, sizeof(int) * 7, c->stream);
    if (e != hipSuccess || cnt <= 0) return e;
    if (!c->temp_unfused) {
        if (maxwell)
            AMC_LAUNCH(c, k_temp_all<AMC_WALL_LAW_MAXWELL>, dim3((unsigned)((cnt + 255) / 256)), dim3(256), c->S, amc_wall_law_params(c),
                               c->out, *cfg, (unsigned int)c->out.step, c->lo, c->hi, D, c->d_cnt);
        else
            AMC_LAUNCH(c, k_temp_all<AMC_WALL_LAW_REFERENCE>, dim3((unsigned)((cnt + 255) / 256)), dim3(256), c->S, c->P, c->out, *cfg,
                               (unsigned int)c->out.step, c->lo, c->hi, D, c->d_cnt);
        return hipGetLastError();
    }
    const unsigned rec_blocks = (unsigned)((D.cap + 255) / 256);
    for (int s = 0; s < 7; s++) {
        const int case_id = 3 + s;
        const size_t o = (size_t)s * (size_t)D.cap;
        temp_records R;
        R.idx = D.idx + o; R.t = D.t + o; R.contact = D.contact + 3 * o; R.normal = D.normal + 3 * o; R.ok = D.ok + o;
        R.count = D.count + s; R.cap = D.cap;
        AMC_LAUNCH(c, k_temp_hits, dim3((unsigned)((cnt + 255) / 256)), dim3(256), c->S, c->P, case_id,
                           c->lo, c->hi, R, c->d_cnt);
        if (maxwell) {
            AMC_LAUNCH(c, k_temp_maxwell, dim3(rec_blocks), dim3(256), c->S, amc_wall_law_params(c), c->out, *cfg, case_id,
                               (unsigned int)c->out.step, R, D.dir + 3 * o, D.Es + o, D.dpz + o, D.dE + o);
            continue;
        }
        AMC_LAUNCH(c, k_temp_sample, dim3(rec_blocks), dim3(256), c->P, *cfg, case_id,
                           (unsigned int)c->out.step, R, D.dir + 3 * o, D.Es + o);
        AMC_LAUNCH(c, k_temp_apply, dim3(rec_blocks), dim3(256), c->S, c->P, c->out, case_id, -1, R,
                           D.dir + 3 * o, D.Es + o, D.dpz + o, D.dE + o, 0, (int *)nullptr, (double *)nullptr);
    }
    return hipGetLastError();
}

// ---- the step's sums on the device (a host-free run, amc_temp_run_device) ------------------------------------------------
// One context's seven record segments as k_case_sums's source (amc_case_sums_dev.h): segment q is case 3 + q.  With ~90 hits
// per case (N = 1e6) ranking is a few hundred LDS reads per thread; a step with more hits than the tile goes through TD.perm.
#define AMC_TEMP_SUMS_TILE 2048
#define AMC_TEMP_SUMS_THREADS 256
struct temp_segments {
    static constexpr int MAX_WORLD = 1;
    temp_dev_segments D;
    struct view {
        const int *idx;
        const unsigned char *okv;
        const double *dpzv, *dEv;
        __device__ int key(int k) const { return idx[k]; }
        __device__ bool ok(int k) const { return okv[k] != 0; }
        __device__ double dpz(int k) const { return dpzv[k]; }
        __device__ double dE(int k) const { return dEv[k]; }
    };
    __device__ int nseg() const { return 7; }
    __device__ int cap() const { return D.cap; }
    __device__ long long count(int q) const { return D.count[q]; }
    __device__ view segment(int q) const
    {
        const size_t o = (size_t)q * (size_t)D.cap;
        return view{D.idx + o, D.ok + o, D.dpz + o, D.dE + o};
    }
};

hipError_t amc_launch_temp_sums(amc_ctx *c, int64_t row)
{
    AMC_LAUNCH(c, (k_case_sums<temp_segments, AMC_TEMP_SUMS_THREADS, AMC_TEMP_SUMS_TILE>), dim3(1), dim3(AMC_TEMP_SUMS_THREADS),
               temp_segments{c->TD.seg}, c->TD.perm, c->TD.series, (int)row, c->TD.ovf, AMC_TEMP_SUMS_TILE);
    return hipGetLastError();
}
