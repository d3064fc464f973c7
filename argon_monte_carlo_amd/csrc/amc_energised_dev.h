// amc_energised_dev.h — the energised wall handlers of Temperature_Pore_MC.py (Temp:349-553) for ONE particle, shared by
// the kernels of amc_energised.hip and by the streaming pass's energised stage (amc_stream.hip, AMC_ST_TEMP_CASES): the
// masks (Temp:708-751), the contact solve, the energy accommodation, the device-side draws (amc_temp_rng) and the
// sequence of all seven cases.
#pragma once
#include "amc_case_sums_dev.h"
#include "amc_philox.h"

__device__ inline bool temp_mask(const amc_params &P, int case_id, double x, double y, double z, double px, double py,
                                 double pz)
{
    const double r2 = x * x + y * y, r02 = px * px + py * py;
    switch (case_id) {
    case 3: return (pz >= P.t_z3_cold) && (z < P.t_z3_cold) && (r2 > P.R_p_sq);                              // Temp:708
    case 4: return (pz <= P.t_z3_hot) && (z > P.t_z3_hot) && (r2 > P.R_p_sq);                                // Temp:713
    case 5: return (pz < P.t_zgap_hi) && (pz > P.t_zgap_lo) && (r02 <= P.R_g_c_sq) && (r2 > P.R_g_c_sq);     // Temp:720
    case 6: return (r02 >= P.R_p_c_sq) && (z < P.t_zgap_lo) && (pz <= P.t_zgap_hi) && (pz >= P.t_zgap_lo);   // Temp:728
    case 7: return (r02 >= P.R_p_c_sq) && (z > P.t_zgap_hi) && (pz <= P.t_zgap_hi) && (pz >= P.t_zgap_lo);   // Temp:734
    case 8: return (r02 <= P.R_p_c_sq) && (r2 > P.R_p_c_sq) && (z <= P.t_zgap_lo) && (z >= P.t_z3_hot);      // Temp:743
    case 9: return (r02 <= P.R_p_c_sq) && (r2 > P.R_p_c_sq) && (z < P.t_z3_cold) && (z > P.t_zgap_hi);       // Temp:749
    default: return false;
    }
}

// contact of a hit of case `case_id`: flight time since contact, contact point, inward unit normal (Temp:349-375 for the
// planes, Temp:430-474 for the cylinders); ok = 0 when the cylinder solve has no real root (Temp:472-474)
struct temp_contact {
    double t, cx, cy, cz, n0, n1, n2;
    unsigned char ok;
};
__device__ inline temp_contact temp_solve(const amc_params &P, int case_id, double x, double y, double z, double vx,
                                          double vy, double vz)
{
    temp_contact c;
    c.ok = 1; c.t = 0; c.cx = 0; c.cy = 0; c.cz = 0; c.n0 = 0; c.n1 = 0; c.n2 = 0;
    if (case_id == 3 || case_id == 4 || case_id == 6 || case_id == 7) {
        const double zp = case_id == 3 ? P.t_z3_cold : case_id == 4 ? P.t_z3_hot : case_id == 6 ? P.t_zgap_lo : P.t_zgap_hi;
        c.t = (z - zp) / vz;                                                                 // Temp:353
        c.cx = x - vx * c.t; c.cy = y - vy * c.t; c.cz = zp;                                 // Temp:372
        c.n2 = (case_id == 3 || case_id == 6) ? 1.0 : -1.0;                                  // Temp:709,714,730,736
    } else {
        const double Rc = case_id == 5 ? P.R_g_c : P.R_p_c;
        const double a = (-vx) * (-vx) + (-vy) * (-vy);                                      // Temp:436
        const double b = 2 * (x * (-vx) + y * (-vy));
        const double cc = x * x + y * y - Rc * Rc;
        const double disc2 = b * b - 4 * a * cc;
        if (a == 0.0 || disc2 < 0.0 || disc2 != disc2) {
            c.ok = 0;                                                                        // Temp:472-474
        } else {
            const double sq = sqrt(disc2);
            const double t1 = (-b + sq) / (2 * a), t2 = (-b - sq) / (2 * a);
            c.t = (t1 < t2) ? t1 : t2;                                                       // Temp:439
            c.cx = x - vx * c.t; c.cy = y - vy * c.t; c.cz = z - vz * c.t;                   // Temp:440
            c.n0 = -(c.cx / Rc); c.n1 = -(c.cy / Rc); c.n2 = -(0.0 / Rc);                    // Temp:442-444 (negated)
        }
    }
    return c;
}

// energy accommodation and new velocity of a hit (Temp:377-388); returns the particle's speed before the hit
__device__ inline double temp_accommodate(const amc_params &P, int case_id, double vx, double vy, double vz, double Es,
                                          double d0, double d1, double d2, double &wvx, double &wvy, double &wvz,
                                          double &dpz, double &dE)
{
    const double m = P.argon_mass;
    const double alpha = (case_id == 5) ? P.alpha_gap : P.alpha_coated;
    const double v_magnitude = sqrt(vx * vx + vy * vy + vz * vz);                            // Temp:377
    const double old_pz = m * vz;                                                            // Temp:378
    const double E = 0.5 * m * (v_magnitude * v_magnitude);                                  // Temp:128-129,379
    const double diff = Es - E;                                                              // Temp:380
    const double Enew = E + diff * alpha;                                                    // Temp:381
    const double mag = sqrt(Enew * 2 / m);                                                   // Temp:383
    dE = Enew - E;                                                                           // Temp:384
    wvx = d0 * mag; wvy = d1 * mag; wvz = d2 * mag;                                          // Temp:386
    dpz = m * wvz - old_pz;                                                                  // Temp:387-388
    return v_magnitude;
}

// ---- opt-in non-parity mode: directions and energies drawn on the device (include/argonmc.h, amc_temp_rng) -----------
// surface_energy_gap (Temp:143-152): 9 T n k (T/theta)^3 * integral_0^{theta/T} x^3/(e^x - 1) dx, Gauss-Legendre
__device__ inline double temp_gap_energy(const amc_temp_rng &g, double z)
{
    const double m = (g.t_cold - g.t_hot) / g.gap_height;                            // Temp:144
    const double t_gap = m * (z - g.gap_bottom_height) + g.t_hot;                    // Temp:145
    const double X = g.t_debye_alumina / t_gap, half = 0.5 * X;
    double q = 0.0;
    for (int i = 0; i < g.n_gl; i++) {
        const double x = half * (g.gl_x[i] + 1.0);
        q += g.gl_w[i] * (x * x * x / expm1(x));
    }
    q *= half;
    const double r = t_gap / g.t_debye_alumina;
    return 9 * t_gap * g.n_alumina * g.boltzman * (r * r * r) * q;                   // Temp:152
}

// re-emission direction (Temp:119-141 recipe on Philox numbers) and surface energy of one hit
__device__ inline void temp_draw(const amc_params &P, const amc_temp_rng &g, int case_id, unsigned int step, int particle,
                                 double n0, double n1, double n2, double contact_z, double &fx, double &fy, double &fz,
                                 double &Es)
{
    // Temp:136's cos(85 * pi / 180) as the reference's Python evaluates it (0.08715574274765814; what p.cos85 and the host
    // helper hold): 2 ulp below the correctly rounded cosine of 85 degrees
    const double cos85 = 0x1.64fd6b8c28100p-4;
    const double pi = 3.14159265358979323846;
    fx = fy = fz = 0;
    for (unsigned int attempt = 0; attempt < 4096u; attempt++) {                     // Temp:133-141 (acceptance ~91 %)
        unsigned int c[4] = {(unsigned int)particle, step, ((unsigned int)case_id << 16) | attempt, 0x414d4331u};
        philox4x32_10(c, g.seed);
        const double u1 = (double)((((unsigned long long)c[0] << 32) | c[1]) >> 11) * (1.0 / 9007199254740992.0);
        const double u2 = (double)((((unsigned long long)c[2] << 32) | c[3]) >> 12) * (1.0 / 4503599627370496.0);
        const double costheta = -1.0 + 2.0 * u1;                                     // Temp:120  U(-1, 1)
        const double phi = pi * u2;                                                  // Temp:121  U(0, pi)
        const double sgn = (c[3] & 1u) ? 1.0 : -1.0;                                 // Temp:124  choice([-1, 1])
        const double theta = acos(costheta);
        fx = cos(phi) * sin(theta);
        fy = sin(phi) * sin(theta) * sgn;
        fz = cos(theta);
        const double d = fma(fz, n2, fma(fy, n1, fx * n0));
        if (fabs(d) < cos85) continue;                                               // Temp:135-136
        if (d < cos85) { fx = -fx; fy = -fy; fz = -fz; }                             // Temp:138-139
        break;
    }
    Es = (case_id == 5) ? temp_gap_energy(g, contact_z)
                        : (amc_case_cold(case_id) ? P.E_cold : P.E_hot);
}

// ---- the Maxwell wall law (include/argonmc-walllaw.h, AMC_WALL_LAW_MAXWELL) -----------------------------------
// New velocity of one hit: with probability alpha a diffuse re-emission from the flux-weighted half-range Maxwellian at the
// local wall temperature, else a specular reflection.  P.alpha_coated / P.alpha_gap are the LAW's two alpha here (the launch
// puts them in place of the reference's accommodation coefficients, which this law does not read).  Es: 2 k T_w for a diffuse
// hit, 0.0 for a specular one.  No rejection loop, no Debye integral.
__device__ inline void temp_maxwell_draw(const amc_params &P, const amc_temp_rng &g, int case_id, unsigned int step, int particle,
                                         double n0, double n1, double n2, double contact_z, double vx, double vy, double vz,
                                         double &wx, double &wy, double &wz, double &Es)
{
    const double pi = 3.14159265358979323846;
    unsigned int w0[4] = {(unsigned int)particle, step, ((unsigned int)case_id << 16) | 0u, 0x414d4332u};
    unsigned int w1[4] = {(unsigned int)particle, step, ((unsigned int)case_id << 16) | 1u, 0x414d4332u};
    philox4x32_10(w0, g.seed);
    const double u0 = (double)((((unsigned long long)w0[0] << 32) | w0[1]) >> 11) * (1.0 / 9007199254740992.0);
    double t_w = amc_case_cold(case_id) ? g.t_cold : g.t_hot;
    if (case_id == 5) {
        const double m = (g.t_cold - g.t_hot) / g.gap_height;                        // as temp_gap_energy forms t_gap
        t_w = m * (contact_z - g.gap_bottom_height) + g.t_hot;
    }
    const double alpha = (case_id == 5) ? P.alpha_gap : P.alpha_coated;
    if (u0 < alpha) {
        philox4x32_10(w1, g.seed);
        const double ua = (double)((((unsigned long long)w0[2] << 32) | w0[3]) >> 11) * (1.0 / 9007199254740992.0);
        const double ub = (double)((((unsigned long long)w1[0] << 32) | w1[1]) >> 11) * (1.0 / 9007199254740992.0);
        const double uc = (double)((((unsigned long long)w1[2] << 32) | w1[3]) >> 11) * (1.0 / 9007199254740992.0);
        const double s = sqrt(g.boltzman * t_w / P.argon_mass);
        const double vn = s * sqrt(-2.0 * log1p(-ua));
        const double rt = s * sqrt(-2.0 * log1p(-ub));
        const double ang = (2.0 * pi) * uc;
        const double t1 = rt * cos(ang), t2 = rt * sin(ang);
        if (case_id == 5 || case_id == 8 || case_id == 9) {                          // cylinders: the normal lies in the xy-plane
            wx = vn * n0 - t1 * n1; wy = vn * n1 + t1 * n0; wz = t2;
        } else {                                                                     // planes: the normal is (0, 0, +-1)
            wx = t1; wy = t2; wz = vn * n2;
        }
        Es = 2 * g.boltzman * t_w;
    } else {
        const double dn = (vx * n0 + vy * n1) + vz * n2;
        const double f = 2.0 * dn;
        wx = vx - f * n0; wy = vy - f * n1; wz = vz - f * n2;
        Es = 0.0;
    }
}

// energies and the recorded direction of a Maxwell hit from the old and the new velocity; returns the speed before the hit
__device__ inline double temp_maxwell_finish(const amc_params &P, double vx, double vy, double vz, double wx, double wy, double wz,
                                             double &d0, double &d1, double &d2, double &dpz, double &dE)
{
    const double m = P.argon_mass;
    const double v_magnitude = sqrt(vx * vx + vy * vy + vz * vz);                            // as temp_accommodate
    const double E = 0.5 * m * (v_magnitude * v_magnitude);
    const double mag = sqrt(wx * wx + wy * wy + wz * wz);
    const double Enew = 0.5 * m * (mag * mag);
    dE = Enew - E;
    dpz = m * wz - m * vz;
    d0 = d1 = d2 = 0.0;
    if (mag != 0.0) { d0 = wx / mag; d1 = wy / mag; d2 = wz / mag; }
    return v_magnitude;
}

// ---- all seven cases of one particle (device-RNG mode) -----------------------------------------------------------------
// Every case reads and writes only the particle itself and the masks are evaluated in case order, each after the
// previous handler ran (Temp:705-758): per particle that is this sequence.  The per-hit records (one segment per case,
// appended in atomic order) are written for the step's sums and for tests.
struct temp_particle {
    double x, y, z, vx, vy, vz, d, dx, dy, dz;
    int flag, nwall, nerr;
};

__device__ inline bool temp_any_mask(const amc_params &P, double x, double y, double z, double px, double py, double pz)
{
    bool any = false;
    for (int case_id = 3; case_id <= 9; case_id++)
        any |= temp_mask(P, case_id, x, y, z, px, py, pz);
    return any;
}

// ROLLED: the form the streaming pass inlines — the case loop stays a loop (one copy of the draw: fewer registers, less code)
// LAW: what a hit does to the velocity (AMC_WALL_LAW_*); everything around the draw is the same under every law
template <bool ROLLED, int LAW = AMC_WALL_LAW_REFERENCE>
__device__ inline void temp_cases_particle(const amc_params &P, const amc_out &O, const amc_temp_rng &g, unsigned int step,
                                           const temp_dev_segments &D, int p, double px, double py, double pz,
                                           temp_particle &q)
{
    double x = q.x, y = q.y, z = q.z, vx = q.vx, vy = q.vy, vz = q.vz;
    double d = q.d, dx = q.dx, dy = q.dy, dz = q.dz;
    bool flag = q.flag != 0;
    int nwall = 0, nerr = 0;
    auto one_case = [&](int case_id) {
        if (!temp_mask(P, case_id, x, y, z, px, py, pz)) return;
        const int s = case_id - 3;
        const int k = atomicAdd(&D.count[s], 1);
        const bool rec = k < D.cap;
        if (!rec) atomicOr(&O.cnt->flags, 4ULL);
        const size_t o = (size_t)s * (size_t)D.cap + (size_t)(rec ? k : 0);
        const temp_contact c = temp_solve(P, case_id, x, y, z, vx, vy, vz);
        double fx = 0, fy = 0, fz = 0, es = 0, dpz = 0, dE = 0;
        nwall++;                                                                             // Temp:411,482,552
        if (!c.ok) {
            nerr++;                                                                          // Temp:472-474
        } else {
            double wvx, wvy, wvz, v_magnitude;
            if constexpr (LAW == AMC_WALL_LAW_MAXWELL) {
                temp_maxwell_draw(P, g, case_id, step, p, c.n0, c.n1, c.n2, c.cz, vx, vy, vz, wvx, wvy, wvz, es);
                v_magnitude = temp_maxwell_finish(P, vx, vy, vz, wvx, wvy, wvz, fx, fy, fz, dpz, dE);
            } else {
                temp_draw(P, g, case_id, step, p, c.n0, c.n1, c.n2, c.cz, fx, fy, fz, es);
                v_magnitude = temp_accommodate(P, case_id, vx, vy, vz, es, fx, fy, fz, wvx, wvy, wvz, dpz, dE);
            }
            if (flag)                                                                        // Temp:391-395
                amc_emit(O, case_id + 1, 0, p, -1, 0, fabs(d - fabs(v_magnitude * c.t)), fabs(dx - fabs(vx * c.t)),
                         fabs(dy - fabs(vy * c.t)), fabs(dz - fabs(vz * c.t)));
            else
                flag = true;
            d = 0; dx = 0; dy = 0; dz = 0;                                                   // Temp:398-401
            x = c.cx; y = c.cy; z = c.cz;                                                    // Temp:402
            vx = wvx; vy = wvy; vz = wvz;                                                    // Temp:403
        }
        if (rec) {
            D.idx[o] = p; D.t[o] = c.t; D.ok[o] = c.ok;
            D.contact[3 * o] = c.cx; D.contact[3 * o + 1] = c.cy; D.contact[3 * o + 2] = c.cz;
            D.normal[3 * o] = c.n0; D.normal[3 * o + 1] = c.n1; D.normal[3 * o + 2] = c.n2;
            D.dir[3 * o] = fx; D.dir[3 * o + 1] = fy; D.dir[3 * o + 2] = fz;
            D.Es[o] = es; D.dpz[o] = dpz; D.dE[o] = dE;
        }
    };
    if (ROLLED) {
#pragma unroll 1
        for (int case_id = 3; case_id <= 9; case_id++) one_case(case_id);
    } else {
        for (int case_id = 3; case_id <= 9; case_id++) one_case(case_id);
    }
    q.x = x; q.y = y; q.z = z; q.vx = vx; q.vy = vy; q.vz = vz;
    q.d = d; q.dx = dx; q.dy = dy; q.dz = dz; q.flag = flag ? 1 : 0;
    q.nwall = nwall; q.nerr = nerr;
}
