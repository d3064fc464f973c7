"""References for the Maxwell wall law of the device-RNG energised pore (include/argonmc-walllaw.h; csrc/amc_energised_dev.h:
temp_maxwell_draw, temp_maxwell_finish) — test infrastructure, CPU only.

* ``uniforms`` — the recipe's four uniforms: two Philox4x32-10 calls (draw_ref.philox) with the counters
  (particle, step, case << 16 | j, "AMC2"), j = 0, 1; u0, ua from words (0, 1) and (2, 3) of call 0, ub, uc of call 1, 53 bits each.
* ``wall_temperature`` / ``emit`` / ``specular`` / ``mirror`` / ``finish`` — the recipe in float64, operation for operation.
* ``reference`` — the recipe with mpmath at 40 digits from the exact uniforms; the decision u0 < alpha is an exact comparison
  of two doubles and is taken as such.  The recipe's constants are its doubles, taken exactly.
``wrong="half_gaussian"`` is a WRONG recipe (vn without the flux weighting), there for tests that show the statistics can tell.
"""
import math

import numpy as np

from tests import draw_ref as R

TAG = 0x414d4332
PI = math.pi
DPS = 40
PLANE_CASES, CYLINDER_CASES, COLD_CASES, GAP_CASE = (3, 4, 6, 7), (5, 8, 9), (3, 7, 9), 5
_U = np.uint64


def _u53(hi, lo):
    return (((hi << _U(32)) | lo) >> _U(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def uniforms(seed, particle, step, case):
    """(u0, ua, ub, uc) per element"""
    case = np.asarray(case).astype(np.uint64)
    w0 = R.philox(particle, step, (case << _U(16)) | _U(0), TAG, seed)
    w1 = R.philox(particle, step, (case << _U(16)) | _U(1), TAG, seed)
    return _u53(w0[0], w0[1]), _u53(w0[2], w0[3]), _u53(w1[0], w1[1]), _u53(w1[2], w1[3])


def wall_temperature(case, contact_z, g):
    """T_w per hit; g: draw_ref.gap_consts(consts).  The gap wall as temp_gap_energy forms t_gap."""
    case = np.asarray(case)
    cz = np.asarray(contact_z, dtype=np.float64)
    m = (g["t_cold"] - g["t_hot"]) / g["gap_height"]
    t_gap = m * (cz - g["bottom"]) + g["t_hot"]
    return np.where(case == GAP_CASE, t_gap, np.where(np.isin(case, COLD_CASES), g["t_cold"], g["t_hot"]))


def emit(ua, ub, uc, s, normal, cylinder, wrong=None, spare=None):
    """the diffuse velocity [n, 3] from the three uniforms, s, the inward normal [n, 3] and the surface kind"""
    ua, ub, uc, s = (np.asarray(a, dtype=np.float64) for a in (ua, ub, uc, s))
    normal = np.asarray(normal, dtype=np.float64)
    vn = s * np.sqrt(-2.0 * np.log1p(-ua))
    if wrong == "half_gaussian":
        vn = vn * np.abs(np.cos((2.0 * PI) * spare))
    rt = s * np.sqrt(-2.0 * np.log1p(-ub))
    ang = (2.0 * PI) * uc
    t1, t2 = rt * np.cos(ang), rt * np.sin(ang)
    n0, n1, n2 = normal[..., 0], normal[..., 1], normal[..., 2]
    cyl = np.stack([vn * n0 - t1 * n1, vn * n1 + t1 * n0, t2], axis=-1)
    pla = np.stack([t1, t2, vn * n2], axis=-1)
    return np.where(np.asarray(cylinder)[..., None], cyl, pla)


def specular(v, normal):
    v, normal = np.asarray(v, dtype=np.float64), np.asarray(normal, dtype=np.float64)
    dn = (v[..., 0] * normal[..., 0] + v[..., 1] * normal[..., 1]) + v[..., 2] * normal[..., 2]
    f = 2.0 * dn
    return v - f[..., None] * normal


def _hits(particle, step, case, normal, contact_z, v):
    particle, step, case = (np.atleast_1d(np.asarray(a)).astype(np.int64) for a in (particle, step, case))
    n = max(len(particle), len(step), len(case))
    particle, step, case = (np.broadcast_to(a, (n,)) for a in (particle, step, case))
    normal = np.broadcast_to(np.asarray(normal, dtype=np.float64), (n, 3))
    v = np.broadcast_to(np.asarray(v, dtype=np.float64), (n, 3))
    cz = np.broadcast_to(np.asarray(contact_z, dtype=np.float64), (n,))
    return n, particle, step, case, normal, cz, v


def mirror(seed, particle, step, case, normal, contact_z, v, alpha_coated, alpha_gap, g, mass, wrong=None):
    """The float64 mirror over arrays of hits: dict with ``w`` [n, 3], ``diffuse``, ``Es``, ``s``, ``t_w`` and the uniforms."""
    n, particle, step, case, normal, cz, v = _hits(particle, step, case, normal, contact_z, v)
    u0, ua, ub, uc = uniforms(seed, particle, step, case)
    t_w = wall_temperature(case, cz, g)
    s = np.sqrt(g["boltzman"] * t_w / mass)
    alpha = np.where(case == GAP_CASE, float(alpha_gap), float(alpha_coated))
    diffuse = u0 < alpha
    w = np.where(diffuse[:, None], emit(ua, ub, uc, s, normal, np.isin(case, CYLINDER_CASES), wrong, u0), specular(v, normal))
    return dict(w=w, diffuse=diffuse, Es=np.where(diffuse, 2 * g["boltzman"] * t_w, 0.0), s=s, t_w=t_w, u0=u0, ua=ua, ub=ub, uc=uc, alpha=alpha)


def finish(v, w, mass):
    """(dir [n, 3], dpz, dE) of the recipe from the old and the new velocity, in float64 as temp_maxwell_finish forms them"""
    v, w = np.asarray(v, dtype=np.float64), np.asarray(w, dtype=np.float64)
    vmag = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
    E = 0.5 * mass * (vmag * vmag)
    mag = np.sqrt(w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1] + w[:, 2] * w[:, 2])
    Enew = 0.5 * mass * (mag * mag)
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.where((mag != 0.0)[:, None], w / mag[:, None], 0.0)
    return d, mass * w[:, 2] - mass * v[:, 2], Enew - E


def reference(seed, particle, step, case, normal, contact_z, v, alpha_coated, alpha_gap, g, mass):
    """The recipe at 40 digits, hit by hit: dict with ``w`` (float64 [n, 3], the reference rounded to double), ``w_lo`` (the
    remainder), ``diffuse``, ``s`` (rounded to double) and ``margin`` = |u0 - alpha|."""
    import mpmath as mp
    n, particle, step, case, normal, cz, v = _hits(particle, step, case, normal, contact_z, v)
    u0, ua, ub, uc = uniforms(seed, particle, step, case)
    out = dict(w=np.zeros((n, 3)), w_lo=np.zeros((n, 3)), diffuse=np.zeros(n, dtype=bool), s=np.zeros(n), margin=np.zeros(n))
    with mp.workdps(DPS):
        f_ = mp.mpf
        k, m, tc, th = f_(g["boltzman"]), f_(float(mass)), f_(g["t_cold"]), f_(g["t_hot"])
        gh, gb, two_pi = f_(g["gap_height"]), f_(g["bottom"]), 2 * f_(PI)
        for h in range(n):
            c = int(case[h])
            t_w = ((tc - th) / gh) * (f_(float(cz[h])) - gb) + th if c == GAP_CASE else (tc if c in COLD_CASES else th)
            s = mp.sqrt(k * t_w / m)
            alpha = float(alpha_gap) if c == GAP_CASE else float(alpha_coated)
            nx, ny, nz = (f_(float(a)) for a in normal[h])
            out["diffuse"][h] = diffuse = bool(u0[h] < alpha)
            out["margin"][h], out["s"][h] = abs(float(u0[h]) - alpha), float(s)
            if diffuse:
                vn = s * mp.sqrt(-2 * mp.log1p(-f_(float(ua[h]))))
                rt = s * mp.sqrt(-2 * mp.log1p(-f_(float(ub[h]))))
                ca, sa = mp.cos_sin(two_pi * f_(float(uc[h])))
                t1, t2 = rt * ca, rt * sa
                w = [vn * nx - t1 * ny, vn * ny + t1 * nx, t2] if c in CYLINDER_CASES else [t1, t2, vn * nz]
            else:
                vx, vy, vz = (f_(float(a)) for a in v[h])
                fdn = 2 * (vx * nx + vy * ny + vz * nz)
                w = [vx - fdn * nx, vy - fdn * ny, vz - fdn * nz]
            hi = [float(a) for a in w]
            out["w"][h] = hi
            out["w_lo"][h] = [float(a - f_(b)) for a, b in zip(w, hi)]
    return out


# ---- the checkpoint's array form (argon_monte_carlo_amd.energised.wall_law_to_array) in plain Python -----------------------------
def law_array(kind, alpha_coated, alpha_gap):
    return np.array([float(kind), float(alpha_coated), float(alpha_gap)], dtype=np.float64)
