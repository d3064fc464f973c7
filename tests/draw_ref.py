"""References for the device-drawn wall directions and gap energies (csrc/amc_energised_dev.h: temp_draw,
temp_gap_energy) — test infrastructure, CPU only.

* ``philox`` — Philox4x32-10 on NumPy arrays (uint64 arithmetic), checked against tests/philox_ref in test_draws_host.py.
* ``uniforms`` / ``mirror`` — temp_draw's recipe in float64, operation for operation: attempt 0, 1, ... with the counter
  (particle, step, case << 16 | attempt, "AMC1"), u1 = 53 bits of words 0 and 1, u2 = 52 bits of words 2 and 3, the sign
  bit 0 of word 3, reject while |d.n| < cos85, flip when d.n < cos85.
* ``reference`` — the same recipe with mpmath at 40 digits from the exact u1, u2 (acos, sin, cos, the dot product with the
  normal); it takes the accept / reject / flip decisions, and reports | |d.n| - cos85 | of every attempt it walks.  The
  recipe's constants are its doubles: cos85 and pi are the values below, taken exactly.
* ``gap_energy_ref`` — surface_energy_gap (Temp:143-152) with mpmath.quad at 40 digits, not through SurfaceEnergies;
  ``gap_energy_gl`` — temp_gap_energy in float64 with leggauss(n_gl).
"""
import math

import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
TAG = 0x414d4331
COS85 = math.cos(85 * math.pi / 180)          # Temp:136: the double this expression yields, 0x1.64fd6b8c28100p-4
PI = math.pi
DPS = 40
MAX_ATTEMPTS = 4096
_U = np.uint64


def philox(c0, c1, c2, c3, seed):
    """Philox4x32-10 of the counters (c0, c1, c2, c3) (broadcast against each other) under the 64-bit seed: four uint64
    arrays holding the 32-bit output words."""
    c = [np.asarray(a).astype(np.uint64) for a in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    m, s32 = _U(0xFFFFFFFF), _U(32)
    for _ in range(10):
        p0, p1 = _U(M0) * c[0], _U(M1) * c[2]
        c = [((p1 >> s32) ^ c[1] ^ _U(k0)) & m, p1 & m, ((p0 >> s32) ^ c[3] ^ _U(k1)) & m, p0 & m]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def uniforms(seed, particle, step, case, attempt, u2_shift=12):
    """(u1, u2, sign, word 3) of one attempt per element.  u2_shift is 12 in the recipe; another value is a WRONG recipe,
    there for tests that show a statistic can tell."""
    case = np.asarray(case).astype(np.uint64)
    w = philox(particle, step, (case << _U(16)) | np.asarray(attempt).astype(np.uint64), TAG, seed)
    u1 = (((w[0] << _U(32)) | w[1]) >> _U(11)).astype(np.float64) * (1.0 / 9007199254740992.0)
    u2 = (((w[2] << _U(32)) | w[3]) >> _U(u2_shift)).astype(np.float64) * (1.0 / float(1 << (64 - u2_shift)))
    sign = np.where((w[3] & _U(1)) != 0, 1.0, -1.0)
    return u1, u2, sign, w[3]


def components(u1, u2, sign):
    """(costheta, phi, unflipped direction [.., 3]) in float64, temp_draw's operations in its order."""
    ct = -1.0 + 2.0 * u1
    phi = PI * u2
    th = np.arccos(ct)
    st = np.sin(th)
    f = np.stack([np.cos(phi) * st, np.sin(phi) * st * sign, np.cos(th)], axis=-1)
    return ct, phi, f


def _fma_dot(f, n):
    # fma(fz, n2, fma(fy, n1, fx * n0)): for the plane normals (0, 0, +-1) that is +-fz exactly; for a cylinder normal
    # n2 == -0.0 and the two roundings of the plain expression differ from the fused ones by an ulp of d at the most
    return f[..., 2] * n[..., 2] + (f[..., 1] * n[..., 1] + f[..., 0] * n[..., 0])


def mirror(seed, particle, step, case, normal, u2_shift=12):
    """The float64 mirror over arrays of hits: dict with ``dir`` [n, 3], ``attempts`` (index of the accepted attempt),
    ``flip`` (bool), ``sign`` (+-1 of the accepted attempt), ``u1``, ``u2`` (of the accepted attempt) and ``walked``: one
    row (hit, attempt, u1, u2, d.n) per attempt walked, in attempt order."""
    particle, step, case = (np.atleast_1d(np.asarray(a)).astype(np.uint64) for a in (particle, step, case))
    n = max(len(particle), len(step), len(case))
    particle, step, case = (np.broadcast_to(a, (n,)) for a in (particle, step, case))
    normal = np.broadcast_to(np.asarray(normal, dtype=np.float64), (n, 3))
    out = dict(dir=np.zeros((n, 3)), attempts=np.zeros(n, dtype=np.int64), flip=np.zeros(n, dtype=bool), sign=np.zeros(n),
               u1=np.zeros(n), u2=np.zeros(n))
    walked = []
    live = np.arange(n)
    for attempt in range(MAX_ATTEMPTS):
        if not len(live):
            break
        u1, u2, sg, _ = uniforms(seed, particle[live], step[live], case[live], attempt, u2_shift)
        _, _, f = components(u1, u2, sg)
        d = _fma_dot(f, normal[live])
        walked.append(np.stack([live.astype(np.float64), np.full(len(live), float(attempt)), u1, u2, d], axis=1))
        acc = ~(np.abs(d) < COS85)
        flip = d < COS85
        a = live[acc]
        out["dir"][a] = np.where(flip[acc][:, None], -f[acc], f[acc])
        out["attempts"][a], out["flip"][a], out["sign"][a] = attempt, flip[acc], sg[acc]
        out["u1"][a], out["u2"][a] = u1[acc], u2[acc]
        live = live[~acc]
    assert not len(live)
    out["walked"] = np.concatenate(walked) if walked else np.zeros((0, 5))
    return out


def _mp():
    import mpmath
    return mpmath


def reference(seed, particle, step, case, normal):
    """The recipe at 40 digits, hit by hit.  dict with ``dir`` (float64 [n, 3]: the reference rounded to double) and
    ``dir_lo`` (the remainder: reference == dir + dir_lo to 1e-32), ``attempts``, ``flip``, ``sign``, ``u1``, ``u2`` as
    in ``mirror``, ``cand`` (per hit the unflipped direction of every attempt walked, float64 [attempts + 1, 3]) and
    ``margins``: one row (hit, attempt, | |d.n| - cos85 |) per attempt walked."""
    mp = _mp()
    particle, step, case = (np.atleast_1d(np.asarray(a)).astype(np.uint64) for a in (particle, step, case))
    n = max(len(particle), len(step), len(case))
    particle, step, case = (np.broadcast_to(a, (n,)) for a in (particle, step, case))
    normal = np.broadcast_to(np.asarray(normal, dtype=np.float64), (n, 3))
    out = dict(dir=np.zeros((n, 3)), dir_lo=np.zeros((n, 3)), attempts=np.zeros(n, dtype=np.int64),
               flip=np.zeros(n, dtype=bool), sign=np.zeros(n), u1=np.zeros(n), u2=np.zeros(n), cand=[None] * n)
    cand = [[] for _ in range(n)]
    margins = []
    live = np.arange(n)
    with mp.workdps(DPS):
        c85, pi = mp.mpf(COS85), mp.mpf(PI)
        nrm = [[mp.mpf(v) for v in row] for row in normal.tolist()]
        for attempt in range(MAX_ATTEMPTS):
            if not len(live):
                break
            u1s, u2s, sgs, _ = uniforms(seed, particle[live], step[live], case[live], attempt)
            keep = []
            for h, u1, u2, sg in zip(live.tolist(), u1s.tolist(), u2s.tolist(), sgs.tolist()):
                cth, sth = mp.cos_sin(mp.acos(-1 + 2 * mp.mpf(u1)))
                cph, sph = mp.cos_sin(pi * mp.mpf(u2))
                f = [cph * sth, sph * sth * int(sg), cth]
                nx, ny, nz = nrm[h]
                d = f[0] * nx + f[1] * ny + f[2] * nz
                margins.append((h, attempt, float(abs(abs(d) - c85))))
                cand[h].append([float(v) for v in f])
                if abs(d) < c85:
                    keep.append(h)
                    continue
                flip = d < c85
                if flip:
                    f = [-v for v in f]
                hi = [float(v) for v in f]
                out["dir"][h] = hi
                out["dir_lo"][h] = [float(v - mp.mpf(a)) for v, a in zip(f, hi)]
                out["attempts"][h], out["flip"][h], out["sign"][h], out["u1"][h], out["u2"][h] = attempt, flip, sg, u1, u2
            live = np.array(keep, dtype=np.int64)
    assert not len(live)
    out["cand"] = [np.array(c) for c in cand]
    out["margins"] = np.array(margins, dtype=np.float64).reshape(-1, 3)
    return out


def implied(dirs, ref, atol):
    """What a set of directions implies, read against the reference's candidates: per hit the (attempt, flip) pairs
    among the attempts the reference walked whose direction lies within atol of dirs (each as a list), and the sign of
    the accepted attempt's y component (0 where |y| <= atol)."""
    pairs, signs = [], []
    for k, c in enumerate(ref["cand"]):
        near = [(a, fl) for a in range(len(c)) for fl in (False, True)
                if np.max(np.abs(dirs[k] - (-c[a] if fl else c[a]))) <= atol]
        pairs.append(near)
        y = dirs[k][1] * (-1.0 if ref["flip"][k] else 1.0)
        signs.append(0.0 if abs(y) <= atol else math.copysign(1.0, y))
    return pairs, np.array(signs)


def u2_bit_statistic(dirs, ref, word3, bit=11):
    """Does the direction depend on a bit of word 3 below the 52 that u2 takes?  Per hit, (dirs - reference) along
    d(direction)/d(phi), divided by pi sin^2(theta), estimates u2(device) - u2(reference); returned is the mean of that
    over the hits with the bit set minus the mean over the hits with it clear, and the number of hits used (those with
    sin(theta) > 1/2).  A recipe that keeps 53 bits shifts the first group by 2^-53 = 1.1e-16; whatever the two groups
    share (the rounding of pi, a libm's bias) cancels."""
    f = ref["dir"]
    diff = (np.asarray(dirs) - f) - ref["dir_lo"]
    s2 = f[:, 0] ** 2 + f[:, 1] ** 2                          # sin^2(theta)
    # d f / d phi of (cos phi sin th, sin phi sin th sgn, cos th) is (-fy sgn, fx sgn, 0), of length sin th; a flip
    # negates f and the derivative alike, so the expression holds for the accepted direction as it stands
    along = (-f[:, 1] * ref["sign"] * diff[:, 0] + f[:, 0] * ref["sign"] * diff[:, 1])
    use = s2 > 0.25
    est = along[use] / (PI * s2[use])
    b = ((np.asarray(word3).astype(np.uint64)[use] >> _U(bit)) & _U(1)) != 0
    return float(est[b].mean() - est[~b].mean()), int(use.sum())


# ---- the gap energy ----------------------------------------------------------------------------------------------------------
def gap_consts(consts):
    return dict(t_cold=consts["t_cold"], t_hot=consts["t_hot"], gap_height=consts["gap_height"],
                bottom=consts["open_air_height"] + consts["hot_coating_height"], debye=consts["t_debye_alumina"],
                n_alumina=consts["num_atoms_unitcell_alumina"], boltzman=consts["boltzman"])


def gap_energy_ref(z, consts):
    """surface_energy_gap(z) (Temp:143-152) at 40 digits: 9 T n k (T/theta)^3 * integral_0^{theta/T} x^3/(e^x - 1) dx with
    mpmath.quad, every constant taken as the double it is.  Returns an mpf."""
    mp = _mp()
    g = gap_consts(consts)
    with mp.workdps(DPS):
        z = mp.mpf(float(z))
        m = (mp.mpf(g["t_cold"]) - mp.mpf(g["t_hot"])) / mp.mpf(g["gap_height"])
        t_gap = m * (z - mp.mpf(g["bottom"])) + mp.mpf(g["t_hot"])
        X = mp.mpf(g["debye"]) / t_gap
        q = mp.quad(lambda x: x ** 3 / mp.expm1(x), [0, X])
        return +(9 * t_gap * mp.mpf(g["n_alumina"]) * mp.mpf(g["boltzman"]) * (t_gap / mp.mpf(g["debye"])) ** 3 * q)


def gap_energy_gl(z, consts, n_gl):
    """temp_gap_energy in float64, operation for operation, with leggauss(n_gl) as device_rng_config fills it in."""
    g = gap_consts(consts)
    xs, ws = np.polynomial.legendre.leggauss(int(n_gl))
    m = (g["t_cold"] - g["t_hot"]) / g["gap_height"]
    t_gap = m * (float(z) - g["bottom"]) + g["t_hot"]
    X = g["debye"] / t_gap
    half = 0.5 * X
    q = 0.0
    for xi, wi in zip(xs.tolist(), ws.tolist()):
        x = half * (xi + 1.0)
        q += wi * (x * x * x / math.expm1(x))
    q *= half
    r = t_gap / g["debye"]
    return 9 * t_gap * g["n_alumina"] * g["boltzman"] * (r * r * r) * q


def rel_err(value, ref):
    """|value / ref - 1| with ref an mpf, as a float"""
    mp = _mp()
    with mp.workdps(DPS):
        return float(abs(mp.mpf(float(value)) / ref - 1))
