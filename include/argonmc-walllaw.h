/* argonmc-walllaw.h — the wall law of the device-RNG energised pore (opt-in).  Included by argonmc.h; the ABI
 * version is argonmc.h's (additions only).
 *
 * What a device-RNG step (amc_temp_cases_device, amc_temp_run_device, the sharded forms) does with a hit of cases 3-9 once the
 * contact is solved.  AMC_WALL_LAW_REFERENCE is the reference's recipe (Temp:119-141, 377-388) on Philox numbers and the
 * default; a context on which amc_temp_wall_law was never called runs exactly that.  AMC_WALL_LAW_MAXWELL is the Maxwell
 * gas-surface model: with probability alpha the molecule leaves diffusely, drawn from the flux-weighted half-range Maxwellian
 * at the local wall temperature (Knudsen's cosine law), otherwise it reflects specularly.
 *
 * The Maxwell recipe for one hit of case `case_id` by particle p in step `step`, inward unit normal n, contact point c,
 * incoming velocity v, m = argon_mass of the context's parameters, k = boltzman and seed of the step's amc_temp_rng (IEEE
 * double as written, no FMA):
 *   Philox4x32-10 under seed, counters (p, step, case_id << 16 | j, 0x414d4332) for j = 0, 1 -> words w0[4], w1[4];
 *   U(hi, lo) = (double)(((uint64)hi << 32 | lo) >> 11) * 2^-53;  u0 = U(w0[0], w0[1]), ua = U(w0[2], w0[3]),
 *   ub = U(w1[0], w1[1]), uc = U(w1[2], w1[3]).  No rejection loop.
 *   T_w = t_cold (cases 3, 7, 9) or t_hot (4, 6, 8); case 5: ((t_cold - t_hot) / gap_height) * (c_z - gap_bottom_height) + t_hot.
 *   s = sqrt(k * T_w / m).  alpha = alpha_gap (case 5) or alpha_coated.  Diffuse iff u0 < alpha.
 *   diffuse:  vn = s * sqrt(-2 * log1p(-ua)), rt = s * sqrt(-2 * log1p(-ub)), ang = (2 pi) * uc, t1 = rt * cos(ang),
 *             t2 = rt * sin(ang);  planes (3, 4, 6, 7): w = (t1, t2, vn * n2);
 *             cylinders (5, 8, 9): w = (vn * n0 - t1 * n1, vn * n1 + t1 * n0, t2).
 *   specular: dn = (vx * n0 + vy * n1) + vz * n2, f = 2 * dn, w = v - f * n.
 *   E = 0.5 * m * (|v| * |v|) as the reference law forms it, mag' = sqrt(wx * wx + wy * wy + wz * wz),
 *   E' = 0.5 * m * (mag' * mag'), dE = E' - E, dpz = m * wz - m * vz.
 * Records (amc_temp_device_draws / _results): dir = w / mag' (zeros when mag' == 0); surface_energy = 2 k T_w for a diffuse
 * hit (the mean energy of the emitted flux) and 0.0 for a specular one; dpz and dE as above.  Completed paths, counters, the
 * failed contact solve, the step's sums and the sampled surfaces are what they are under the reference law.
 *
 * The law is host state of the context: it applies to the next device-RNG step of any form, not to the host-RNG hand-over
 * (amc_temp_begin -> amc_wall_hits -> amc_wall_apply).  amc_reset_outputs leaves it alone.  Setting it allocates nothing. */
#ifndef ARGONMC_WALLLAW_H
#define ARGONMC_WALLLAW_H
#define AMC_WALL_LAW_REFERENCE 0      /* Temp:119-141, 377-388 on Philox numbers */
#define AMC_WALL_LAW_MAXWELL   1
typedef struct amc_wall_law {
    int32_t struct_size, kind;        /* sizeof(amc_wall_law); AMC_WALL_LAW_*                                                 */
    double  alpha_coated, alpha_gap;  /* MAXWELL: probability of a diffuse re-emission on the coated surfaces / the gap wall,
                                         in [0, 1]                                                                            */
    double  reserved[4];              /* 0 */
} amc_wall_law;
/* NULL: back to AMC_WALL_LAW_REFERENCE.  AMC_ERR_STATE unless the context is an energised pore; AMC_ERR_INVALID (the law in
 * force stays) for a bad struct_size or kind, an alpha outside [0, 1] or NaN, or a non-zero reserved word. */
int amc_temp_wall_law(amc_ctx *ctx, const amc_wall_law *law);
/* the law in force (the reference law reads kind 0 and the context parameters' alpha_coated / alpha_gap) */
int amc_temp_wall_law_get(amc_ctx *ctx, amc_wall_law *out);
#endif /* ARGONMC_WALLLAW_H */
