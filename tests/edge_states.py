"""Crafted states that put particles exactly on the decision points of the hot path: wall planes and cylinders, the
bounds thresholds, reference-cell faces, detection-grid faces, histogram edges and field-bin edges.

Pure NumPy and deterministic (no random numbers at all).  Every builder returns an ``EdgeState``: the full state to upload
(positions, velocities, d, dx, dy, dz, flag), the params and dt it is meant for, and ``cases`` — the name of every edge case
it contains with the particle indices that carry it, so that a test can check each case is really exercised.

Positions that must sit on an edge AFTER the drift are "landed": the uploaded coordinate is chosen so that the drift's own
arithmetic, ``v0 + dt * vel``, rounds to the edge value exactly.
"""
from __future__ import annotations

import numpy as np

from argon_monte_carlo_amd import params as PR

TINY = np.nextafter(0.0, 1.0)
STATE = ["x", "y", "z", "vx", "vy", "vz", "d", "dx", "dy", "dz"]


def around(v, k=2):
    """v, its neighbours 1 .. k ulp below and above (ascending)."""
    v = np.float64(v)
    lo, hi = [v], [v]
    for _ in range(k):
        lo.append(np.nextafter(lo[-1], -np.inf))
        hi.append(np.nextafter(hi[-1], np.inf))
    return [float(a) for a in lo[:0:-1] + [v] + hi[1:]]


def land(target, vel, dt):
    """A start coordinate v0 with fl(v0 + fl(dt * vel)) == target (the drift's arithmetic), or None."""
    s = np.float64(dt) * np.float64(vel)
    v0 = np.float64(target) - s
    cand = [v0]
    a = b = v0
    for _ in range(8):
        a, b = np.nextafter(a, -np.inf), np.nextafter(b, np.inf)
        cand += [a, b]
    for c in cand:
        if c + s == np.float64(target):
            return float(c)
    return None


class EdgeState:
    """A crafted state: arrays ``x .. dz`` (float64), ``flag`` (uint8), ``p`` (AmcParams with p.n set), ``dt`` and
    ``cases`` {name: [particle index, ...]}."""

    def __init__(self, p, dt):
        self.p, self.dt = p, float(dt)
        self._rows = []
        self.cases = {}
        self.extra = {}

    def add(self, case, x, y, z, vx, vy, vz, d=1.0e-8, dx=6.0e-9, dy=5.0e-9, dz=4.0e-9, flag=1, landed=True,
            jitter=True):
        """Append one particle.  With landed=True (x, y, z) is where the particle must be AFTER the drift; returns its
        index, or None if no start coordinate lands exactly there.  jitter adds a per-particle 1e-3 m/s to a non-zero vx."""
        pos = [x, y, z]
        if jitter and vx != 0.0:
            vx = vx + 1.0e-3 * (len(self._rows) % 997)      # (no two particles share a velocity: a == 0 only by design)
        if landed:
            pos = [land(t, v, self.dt) for t, v in zip((x, y, z), (vx, vy, vz))]
            if any(c is None for c in pos):
                return None
        i = len(self._rows)
        self._rows.append([float(v) for v in pos + [vx, vy, vz, d, dx, dy, dz]] + [int(flag)])
        self.cases.setdefault(case, []).append(i)
        return i

    def finish(self):
        a = np.array(self._rows, dtype=np.float64).reshape(-1, 11)
        for k, name in enumerate(STATE):
            setattr(self, name, np.ascontiguousarray(a[:, k]))
        self.flag = np.ascontiguousarray(a[:, 10].astype(np.uint8))
        self.p.n = len(a)
        return self

    @property
    def n(self):
        return len(self.x)

    def arrays(self):
        """the 10 state arrays and the flag, in upload order (copies)"""
        return [getattr(self, k).copy() for k in STATE] + [self.flag.copy()]


# ---------------------------------------------------------------------------------------------------------- pore walls
def _pore():
    p, c = PR.pore_params(n=0)
    return p, c


def pore_walls(fp_cases=False):
    """Particles on every plane and cylinder the pore's wall cases (Pore:439-485) compare against.

    fp_cases adds side-wall solves without a real root (a == 0, a negative discriminant): those need reserved1 bit0
    (count and continue), otherwise the step fails like the reference does."""
    p, c = _pore()
    dt = c["dt"]
    s = EdgeState(p, dt)
    zb, zt = p.z_gap_bottom, p.z_gap_top
    planes = dict(zero=0.0, H=p.H, z_cold=p.z_cold, h_oa=p.h_oa, z_gap_bottom=zb, z_gap_top=zt)
    # (x, y) spots 1.2 nm apart — more than three collision ranges — inside the pore (every plane is open there) and over
    # the coatings / in the gap (the planes of cases 3 and 5); a fresh set per plane, the planes being far apart
    def spots(rmin, rmax):
        g = np.arange(-rmax, rmax + 1e-12, 1.2e-9)
        X, Y = np.meshgrid(g, g, indexing="ij")
        R = np.hypot(X, Y)
        ok = (R > rmin) & (R < rmax)
        return list(zip(X[ok].tolist(), Y[ok].tolist()))

    for pname, zp in planes.items():
        for rname, (rmin, rmax) in dict(pore=(3e-9, p.R_p - 4e-9), coat=(p.R_p + 0.8e-9, p.R_g - 0.8e-9)).items():
            if rname == "coat" and pname in ("zero", "H"):
                continue
            sp = iter(spots(rmin, rmax))
            for zv in around(zp):
                for vz in (-431.0, 431.0):
                    # current z on (or next to) the plane
                    s.add(f"cur_z_{pname}", *next(sp), zv, 97.0, -61.0, vz)
                    # prior z on the plane: uploaded there, the drift moves it off
                    s.add(f"prior_z_{pname}", *next(sp), zv, 97.0, -61.0, vz, landed=False)
    slot = [0]
    inner = spots(3e-9, 20e-9)
    sp0, sp1 = iter(inner[::2]), iter(inner[1::2])

    def xy(r, diag):
        return next(sp1 if diag else sp0)

    # vz = +-0.0 with z exactly on 0 and H; the smallest |vz| with z just below 0 (t = z / vz stays finite)
    for zp, name in ((0.0, "zero"), (p.H, "H")):
        for vz in (0.0, -0.0):
            x, y = xy(None, False)
            s.add(f"vz0_on_{name}", x, y, zp, 50.0, 20.0, vz)
    for k in (1, 3, 1 << 20):
        for vz in (-TINY, TINY):
            x, y = xy(None, True)
            s.add("tiny_vz_below_zero", x, y, -k * TINY, 0.0, 0.0, vz, landed=False)
    # radii exactly on R_oa (open air), R_g (gap), R_p (pore body and gap), current and prior, axis and diagonal
    zc = dict(R_oa=0.5 * p.h_oa, R_g=0.5 * (zb + zt), R_p=0.5 * (p.h_oa + zb))
    for name, R in (("R_oa", p.R_oa), ("R_g", p.R_g), ("R_p", p.R_p)):
        zs = [zc[name]] + ([0.5 * (zb + zt), 0.5 * (zt + p.z_cold)] if name == "R_p" else [])
        for z in zs:
            for rv in around(R):
                for vr in (-300.0, 300.0):
                    slot[0] += 1
                    off = slot[0] * 1.0e-9                                  # (keeps particles apart in z)
                    s.add(f"cur_r_{name}", rv, 0.0, z + off, vr, 0.0, 40.0)
                    s.add(f"prior_r_{name}", rv, 0.0, z + off + 0.5e-9, vr, 0.0, 40.0, landed=False)
                    h = rv / np.sqrt(2.0)
                    s.add(f"cur_r_{name}_diag", h, h, z + off + 0.25e-9, vr, vr, 40.0)
    # corner crossings: across R_g and z_gap_bottom / z_gap_top in one step (case 4 then case 5), across R_p and
    # z_gap_bottom (case 5 and 6), across z_cold beside the pore mouth
    vfast = 2600.0
    step = vfast * dt

    def rot(name, x, y, z, vx, vy, vz):
        # (cylinders are round: turning position and velocity together keeps the case; each particle its own azimuth)
        slot[0] += 1
        a = 0.07 * slot[0]
        ca, sa = np.cos(a), np.sin(a)
        s.add(name, ca * x - sa * y, sa * x + ca * y, z, ca * vx - sa * vy, sa * vx + ca * vy, vz, landed=False,
              jitter=False)

    for j, (zplane, sgn) in enumerate(((zb, -1.0), (zt, 1.0))):
        for q in range(6):
            frac = 0.15 + 0.14 * q
            z0 = zplane - sgn * (1.0 - frac) * step * 0.5
            rot("corner_Rg_gap", p.R_g - frac * step, 0.0, z0, vfast, 0.0, sgn * vfast)
            rot("corner_Rp_gap", p.R_p + frac * step, 0.0, z0, -vfast, 0.0, sgn * vfast)
    for q in range(6):
        frac = 0.15 + 0.14 * q
        rot("corner_cold_mouth", p.R_p - frac * step, 0.0, p.z_cold + (1.0 - frac) * step * 0.5, vfast, 0.0, -vfast)
        rot("corner_hot_mouth", p.R_p - frac * step, 0.0, p.h_oa - (1.0 - frac) * step * 0.5, vfast, 0.0, vfast)
    # tangential solves on the R_oa_c cylinder (case 1): y = R_oa_c, vy = 0, vx a power of two; disc2 = 2^18 (x^2 - c)
    # with c = fl(fl(x^2) + R_oa_c^2) - R_oa_c^2, so it is exactly 0, or positive / negative by rounding, depending on x
    Rc = p.R_oa_c
    x_t = np.sqrt(p.R_oa ** 2 - Rc ** 2) * 1.0005
    found = {"tangent_disc0": 0, "tangent_disc_pos": 0, "tangent_disc_neg": 0}
    xv = np.float64(x_t)
    for _ in range(400):
        xv = np.nextafter(xv, np.inf)
        for vx in (256.0, -256.0):
            a = vx * vx
            b = 2 * (xv * (-vx) + Rc * (-0.0))
            cc = xv * xv + Rc * Rc - Rc * Rc
            disc = b * b - 4 * a * cc
            key = "tangent_disc0" if disc == 0 else ("tangent_disc_pos" if disc > 0 else "tangent_disc_neg")
            if found[key] >= 3 or (key == "tangent_disc_neg" and not fp_cases):
                continue
            if s.add(key, float(xv), Rc, 0.3 * p.h_oa + found[key] * 1e-9 + (vx > 0) * 5e-9, vx, 0.0, 100.0,
                     jitter=False) is not None:
                found[key] += 1
    if fp_cases:
        # a == 0: outside R_oa with no radial motion at all (+-0.0)
        for vx, vy in ((0.0, 0.0), (-0.0, 0.0), (0.0, -0.0)):
            s.add("side_a0", p.R_oa * 1.01, 3.0e-9 * len(s.cases.get("side_a0", [])), 0.4 * p.h_oa, vx, vy, 200.0)
        # grazing R_g: the line from prior to current passes between R_g_c and R_g -> no real root (case 4)
        # and the same past R_p between R_p_c and R_p (case 6)
        for name, R, Rcc, zz in (("graze_Rg", p.R_g, p.R_g_c, 0.5 * (zb + zt)), ("graze_Rp", p.R_p, p.R_p_c, 0.5 * (p.h_oa + zb))):
            y = 0.5 * (R + Rcc)
            xc = np.sqrt(R * R - y * y)
            for q in range(3):
                rot(name, xc - 0.3 * step, y, zz, vfast, 0.0, 10.0)
    return s.finish()


def pore_bounds():
    """Positions (after drift and walls) on the thresholds of num_out_of_bounds (Pore:354-375): z on 0 and H, x*x + y*y
    on R_oa_sq, R_g_sq and R_p_sq (as near as doubles allow) at z on each threshold of the radial tests."""
    p, c = _pore()
    s = EdgeState(p, c["dt"])
    for zv in around(0.0) + around(p.H):
        s.add("z_lo_hi", 5.0e-9, 3.0e-9 * len(s.cases.get("z_lo_hi", [])), zv, 0.0, 0.0, 0.0)
    zs = dict(h_oa=p.h_oa, z_cold=p.z_cold, z_oob_hot_top=p.z_oob_hot_top, z_oob_gap_top=p.z_oob_gap_top)
    for rname, Rsq in (("R_oa_sq", p.R_oa_sq), ("R_g_sq", p.R_g_sq), ("R_p_sq", p.R_p_sq)):
        r0 = np.sqrt(Rsq)
        q = 0
        for zname, zt in zs.items():
            for zv in around(zt, 1):
                for want in ("below", "on", "above"):
                    # each particle at its own azimuth (arc steps of ~ 3 collision ranges); x moved by ulps until
                    # x*x + y*y falls on the wanted side of the threshold (or on it, where some x gets there)
                    q += 1
                    ang = q * 3.0e-9 / r0
                    y = r0 * np.sin(ang)
                    best = r0 * np.cos(ang)
                    for xv in around(r0 * np.cos(ang), 6):
                        v = xv * xv + y * y
                        side = "on" if v == Rsq else ("above" if v > Rsq else "below")
                        if side == want:
                            best = xv
                            break
                    case = rname if q % 2 else rname + "_diag"
                    if q % 2 == 0:                # (the diagonal: turned by 45 degrees, the same radius)
                        c45 = np.sqrt(0.5)
                        s.add(case, c45 * (best - y), c45 * (best + y), zv, 0.0, 0.0, 0.0)
                    else:
                        s.add(case, best, y, zv, 0.0, 0.0, 0.0)
    return s.finish()


# ---------------------------------------------------------------------------------------------------------- cube walls
def _cube(side=100.0e-9, n_sub=15):
    p, c = PR.cube_params(n=0, cube_side=side, n_sub=n_sub)
    return p, c


def cube_walls():
    """Positions exactly on 0 and cube_* (and next to them), +-0.0 velocities, particles that cross both walls of one axis
    in one step (Cube:189-226)."""
    p, c = _cube()
    dt = c["dt"]
    s = EdgeState(p, dt)
    W = (p.cube_x, p.cube_y, p.cube_z)
    mid = 0.5 * p.cube_x
    k = 0
    for ax in range(3):
        for wall, wv in (("lo", 0.0), ("hi", W[ax])):
            for v in around(wv):
                for vel in (-350.0, 350.0, 0.0, -0.0):
                    if vel == 0.0 and v != wv:
                        continue                  # (a zero velocity off the wall: t = +-inf, not a state the reference reaches)
                    k += 1
                    pos = [mid + 1.3e-9 * (k % 40), mid - 1.1e-9 * (k // 40), mid + 0.9e-9 * (k % 7)]
                    vv = [30.0, -20.0, 10.0]
                    pos[ax], vv[ax] = v, vel
                    s.add(f"on_{'xyz'[ax]}_{wall}", *pos, *vv)
        # both walls of one axis in one step: from inside, beyond the far wall by more than the cube's width
        for q, f in enumerate((2.5, 2.25, 2.75)):
            for sgn in (1.0, -1.0):
                vv = [10.0, 10.0, 10.0]
                pos = [mid + 2e-9 * q, mid - 2e-9 * q, mid + 3e-9 * (ax + 1)]
                vv[ax] = sgn * (f - 0.5) * W[ax] / dt * 0.999
                s.add(f"both_walls_{'xyz'[ax]}", *pos, *vv, landed=False)
    return s.finish()


# ---------------------------------------------------------------------------------------------------------- reference cells
def _cell_layout(p, kind):
    """per axis: (d, ov, list of k whose faces k*d - ov and (k+1)*d bound a cell, offset making k a layer index)"""
    if kind == "pore":
        nxy = p.nx
        return [(p.dx, p.overlap_x, nxy), (p.dy, p.overlap_y, nxy), (p.dz, p.overlap_z, 0)]
    return [(p.dx, p.overlap_x, 0), (p.dy, p.overlap_y, 0), (p.dz, p.overlap_z, 0)]


def cell_pairs(kind, for_timestep=True):
    """Colliding pairs of particles on the faces of the reference cells (Pore:520-530 / Cube:231-240): one particle on
    k*d - ov or (k+1)*d (and 1, 2 ulp either side), its partner half a collision range into the overlap strip, for every
    axis, every colour group (the parities of the three axes) and the first and last layers."""
    if kind == "pore":
        p, c = _pore()
    else:
        p, c = _cube()
    dt = c["dt"]
    s = EdgeState(p, dt)
    cr = p.collision_range
    lay = _cell_layout(p, kind)
    nk = [p.nx, p.ny, p.nz]
    vrel = 200.0
    pairs = []
    for ax in range(3):
        d, ov, off = lay[ax]
        # k of the first and last layers, their neighbours and two in the middle (both parities everywhere)
        if kind == "pore" and ax < 2:
            ks = [-off, -off + 1, -1, 0, nk[ax] - off - 2, nk[ax] - off - 1]
        else:
            ks = [0, 1, nk[ax] // 2, nk[ax] // 2 + 1, nk[ax] - 2, nk[ax] - 1]
        o1, o2 = [a for a in range(3) if a != ax]
        for k in sorted(set(ks)):
            faces = []
            lo_face = np.float64(k) * d - ov
            hi_face = np.float64(k + 1) * d
            if k != ks[0] or kind == "cube":
                faces.append(("lo", lo_face))
            if k != ks[-1] or kind == "cube":
                faces.append(("hi", hi_face))
            for fname, face in faces:
                if kind == "cube" and (face <= cr or face >= nk[ax] * d - cr):
                    continue                      # (on the cube's own walls)
                for par1 in (0, 1):
                    for par2 in (0, 1):
                        # the other two coordinates: mid-cell in a cell of the wanted parity, away from every face
                        oc = []
                        for oa, par in ((o1, par1), (o2, par2)):
                            do, ovo, offo = lay[oa]
                            if kind == "pore" and oa < 2:
                                kk = -1 + par                   # cells -1 / 0: |coordinate| < dx, inside R_p
                            elif kind == "pore":
                                kk = (1 if ax < 2 else 60) + par        # z: bottom open air for x/y pairs, body for z pairs
                            else:
                                kk = 6 + par
                            oc.append((oa, kk * do + 0.2 * do))
                        for j, fv in enumerate(around(face)):
                            # (the variants 3 collision ranges apart along o1, the lo and hi faces of one plane along o2:
                            # a lo face k*d - ov and the hi face k*d of the cell below are only ov apart)
                            pos = [0.0, 0.0, 0.0]
                            for oa, ov_ in oc:
                                pos[oa] = ov_ + 3.0 * cr * j * (1 if oa == o1 else 0)
                            pos[o2] += 3.0 * cr if fname == "lo" else 0.0
                            pa = list(pos)
                            pb = list(pos)
                            pa[ax] = fv
                            sgn = 1.0 if fname == "lo" else -1.0
                            pb[ax] = fv + sgn * 0.5 * cr
                            va = [0.0, 0.0, 0.0]
                            vb = [0.0, 0.0, 0.0]
                            va[ax], vb[ax] = sgn * vrel, -sgn * vrel
                            va[o1] = vb[o1] = 13.0
                            if kind == "pore" and ax < 2:
                                rr = np.hypot(*[pa[a] for a in range(2)])
                                if rr >= p.R_oa - cr:
                                    continue
                            ia = s.add(f"cell_{'xyz'[ax]}_{fname}", *pa, *va, landed=for_timestep)
                            if ia is None:
                                continue
                            ib = s.add(f"cell_{'xyz'[ax]}_{fname}", *pb, *vb, landed=for_timestep)
                            if ib is None:
                                s._rows.pop()
                                s.cases[f"cell_{'xyz'[ax]}_{fname}"].pop()
                                continue
                            grp = ((int(np.floor(pa[0] / lay[0][0])) + lay[0][2]) & 1,
                                   (int(np.floor(pa[1] / lay[1][0])) + lay[1][2]) & 1,
                                   (int(np.floor(pa[2] / lay[2][0])) + lay[2][2]) & 1)
                            s.cases.setdefault(f"group_{grp[0]}{grp[1]}{grp[2]}", []).append(ia)
                            if k in (ks[0], ks[-1]):
                                s.cases.setdefault("first_last_layer", []).append(ia)
                            pairs.append((ia, ib))
    s.extra["pairs"] = np.array(pairs, dtype=np.int64).reshape(-1, 2)
    return s.finish()


def cell_chains(n_chain=14):
    """Pore: chains of n_chain particles 0.8 collision ranges apart lying IN a reference-cell face (x or z exactly on
    k*d - ov or (k+1)*d), so that the whole chain is one cluster of more than 11 members — the size at which the resolve
    stops emulating clusters from cached cell indices and tests every member's cells again (amc_axis_cell)."""
    p, c = _pore()
    dt = c["dt"]
    s = EdgeState(p, dt)
    cr = p.collision_range
    for q, (ax, face, along) in enumerate(((0, -1 * p.dx - p.overlap_x, 1), (0, 1 * p.dx, 1), (0, 0 * p.dx - p.overlap_x, 2),
                                            (2, 60 * p.dz - p.overlap_z, 0), (2, 61 * p.dz, 1), (2, 75 * p.dz - p.overlap_z, 0))):
        base = [-0.5 * p.dx + 0.21 * p.dx, -0.5 * p.dx + 0.17 * p.dx, 60.4 * p.dz + 0.13 * q * p.dz]
        base[ax] = float(face)
        if ax == 0:
            base[2] = 30.3 * p.dz + 2.1 * q * p.dz
        for m in range(n_chain):
            pos = list(base)
            pos[along] = base[along] + 0.8 * cr * m
            v = [0.0, 0.0, 0.0]
            v[along] = 150.0 if m % 2 else -150.0
            v[3 - ax - along] = 20.0 * (m % 3)
            s.add(f"chain_{'xyz'[ax]}", *pos, *v)
    return s.finish()


# ---------------------------------------------------------------------------------------------------------- detection grid
SEP_M = (1, 2, 3, 8)


def _separations(cr):
    """(name, separation): just inside collision_range by m * 2^-52 relative, exactly on it, just above it"""
    out = [(f"in_{m}", cr * (1.0 - m * 2.0 ** -52)) for m in SEP_M]
    out += [("on", cr), ("above_1", float(np.nextafter(cr, np.inf))), ("above_far", cr * (1.0 + 1e-9))]
    return out


def distance_lt(ax, ay, az, bx, by, bz, cr):
    """the overlap test of Pore:173-174 in the kernels' arithmetic (exact squares)"""
    ex, ey, ez = bx - ax, by - ay, bz - az
    return np.sqrt(ex * ex + ey * ey + ez * ez) < cr


def grid_pairs(kind, fine_cell_mult=2.01 * 1.02, for_timestep=True):
    """Approaching pairs at separations around collision_range across faces, edges and corners of the detection grid
    (fine_cell = fine_cell_mult * collision_range, faces at xlo - h + k h), at the domain corner farthest from the origin,
    at the edge of the pore's narrow layer windows, and (for_timestep=False) just outside the domain.

    extra["pairs"]: (i, j) per pair; extra["collide"]: whether the pair overlaps in the kernels' arithmetic at the sweep."""
    if kind == "pore":
        p, c = _pore()
        xlo, xhi, zhi = -p.R_oa, p.R_oa, p.H
    else:
        p, c = _cube()
        xlo, xhi, zhi = 0.0, p.cube_x, p.cube_z
    dt = c["dt"]
    cr = p.collision_range
    h = fine_cell_mult * cr
    p.fine_cell = h
    p.detect_mode = 1
    x0 = xlo - h
    z0 = 0.0 - h
    s = EdgeState(p, dt)
    pairs, collide = [], []

    def face(o, v):                      # the grid face at or below v
        return o + np.floor((v - o) / h) * h

    # anchors: grid points (faces on all three axes) — mid domain, near the far corner, in the pore body at the window edge
    anchors = []
    if kind == "cube":
        anchors.append(("mid", face(x0, 0.5 * xhi), face(x0, 0.5 * xhi), face(z0, 0.5 * zhi)))
        anchors.append(("far_corner", face(x0, xhi - 12 * h), face(x0, xhi - 2 * h), face(z0, zhi - 12 * h)))
    else:
        anchors.append(("mid", face(x0, 0.0), face(x0, 0.0), face(z0, 0.5 * p.h_oa)))
        r_far = 0.6 * p.R_oa
        anchors.append(("far_corner", face(x0, r_far), face(x0, r_far), face(z0, zhi - 12 * h)))
        # inside the pore body next to the narrowed window: the face nearest to R_g in x, the gap's mid z
        anchors.append(("window_edge", face(x0, p.R_g - 2 * cr), face(x0, 0.0), face(z0, 0.5 * (p.z_gap_bottom + p.z_gap_top))))
    dirs = dict(face=(1.0, 0.0, 0.0), edge=(1.0, 1.0, 0.0), corner=(1.0, 1.0, 1.0))
    vrel = 150.0
    slot = 0
    for aname, ax_, ay_, az_ in anchors:
        for dname, dv in dirs.items():
            u = np.array(dv) / np.linalg.norm(dv)
            for sname, sep in _separations(cr):
                slot += 1
                # spread the pairs along the face (y for 'face', z otherwise) so that they stay apart; the pair straddles
                # the anchor point, i.e. the face / edge / corner of the grid cells
                ctr = np.array([ax_, ay_, az_])
                a = ctr - 0.5 * sep * u
                b = a + sep * u
                if dname == "face":
                    a[2] = b[2] = ctr[2] + (slot % 16) * 3.1 * cr - 8 * 3.1 * cr + 0.37 * h
                    a[1] = b[1] = ctr[1] + 0.41 * h
                elif dname == "edge":
                    a[2] = b[2] = ctr[2] + (slot % 16) * 3.1 * cr - 8 * 3.1 * cr + 0.33 * h
                else:
                    # corners: one pair per corner point, three cells over in y (away from the face pairs), walking along
                    # the z faces
                    off = ((slot % 16) - 8) * h
                    a[1] += 3 * h
                    b[1] += 3 * h
                    a[2] += off
                    b[2] += off
                va = -u * vrel * 0.5
                vb = u * vrel * 0.5                # separating slowly: overlap decides, the solve stays regular
                va[1] += 7.0
                vb[1] += 7.0
                va[2] += 3.0
                vb[2] += 3.0
                ia = s.add(f"grid_{aname}_{dname}_{sname}", *a, *va, landed=for_timestep)
                ib = s.add(f"grid_{aname}_{dname}_{sname}", *b, *vb, landed=for_timestep)
                if ia is None or ib is None:
                    raise AssertionError(f"cannot land the pair {aname} {dname} {sname}")
                pairs.append((ia, ib))
    s.extra["pairs"] = np.array(pairs, dtype=np.int64).reshape(-1, 2)
    st = s.finish()
    # the positions the sweep sees: after the drift (the same arithmetic), or as uploaded
    if for_timestep:
        X = [st.x + dt * st.vx, st.y + dt * st.vy, st.z + dt * st.vz]
    else:
        X = [st.x, st.y, st.z]
    P = st.extra["pairs"]
    st.extra["collide"] = distance_lt(X[0][P[:, 0]], X[1][P[:, 0]], X[2][P[:, 0]], X[0][P[:, 1]], X[1][P[:, 1]],
                                      X[2][P[:, 1]], cr)
    return st


def outside_pairs():
    """pore pairs just outside the domain (below z = 0 by less / more than one grid cell, beyond R_oa): for a sweep run
    before walls and bounds act on them"""
    p, c = _pore()
    cr = p.collision_range
    h = 2.01 * 1.02 * cr
    p.fine_cell = h
    p.detect_mode = 1
    s = EdgeState(p, c["dt"])
    pairs = []
    for q, (x, y, z) in enumerate([(1e-9, 2e-9, -0.3 * cr), (4e-9, 2e-9, -0.6 * h), (8e-9, 2e-9, -1.5 * h),
                                   (p.R_oa + 0.2 * cr, 0.0, 0.5 * p.h_oa), (0.0, p.R_oa + 2.5 * h, 0.3 * p.h_oa),
                                   (1.5e-8, 1.1e-8, p.H + 0.4 * cr), (-1.5e-8, 1.1e-8, p.H + 2.2 * h)]):
        for j, m in enumerate((1, 0)):
            sep = cr * (1.0 - m * 2.0 ** -52) if m else cr * 0.5
            a = np.array([x, y + 4 * cr * j, z])
            b = a + np.array([0.0, 0.0, sep]) if q < 3 or q >= 5 else a + np.array([sep, 0.0, 0.0])
            ia = s.add(f"outside_{q}", *a, 0.0, 5.0, 80.0, landed=False)
            ib = s.add(f"outside_{q}", *b, 0.0, 5.0, -80.0, landed=False)
            pairs.append((ia, ib))
    s.extra["pairs"] = np.array(pairs, dtype=np.int64)
    return s.finish()


# ---------------------------------------------------------------------------------------------------------- histograms
# the default range, a non-dyadic one with 7 bins, a single bin, and two where exact edges need the fix-up's up move
HIST_RANGES = [(0.0, 1.0e-6, 200), (1.3e-8, 7.7e-7, 7), (2.0e-9, 3.0e-7, 1), (1.0e-9, 1.0e-6, 200), (1.3e-8, 7.7e-7, 5)]

def hist_values(lo, hi, nbins, k=2):
    """Values aimed at np.histogram's decisions: every edge of np.linspace(lo, hi, nbins + 1) with its neighbours up to k
    ulp, lo and hi, values just outside, +inf and -0.0.  Only values >= 0 (a wall hit emits |dx|)."""
    edges = np.linspace(lo, hi, nbins + 1)
    vals = []
    for e in edges:
        vals += around(e, k)
    vals += [lo, hi, float(np.nextafter(hi, np.inf)), hi * 1.5 + 1e-9, np.inf, -0.0]
    if lo > 0:
        vals += [float(np.nextafter(lo, -np.inf)), 0.5 * lo]
    v = np.array([a for a in vals if a >= 0 or (a == 0 and np.signbit(a))], dtype=np.float64)
    return v


def hist_guess(v, lo, hi, nbins):
    """the kernel's first guess int(((v - lo) / (hi - lo)) * nbins), with nbins -> nbins - 1 (finite in-range v only)"""
    g = (((v - lo) / (hi - lo)) * nbins).astype(np.int64)
    g[g == nbins] -= 1
    return g


def hist_true_bin(v, lo, hi, nbins):
    """the bin np.histogram puts each in-range value in"""
    edges = np.linspace(lo, hi, nbins + 1)
    b = np.searchsorted(edges, v, side="right") - 1
    b[v == hi] = nbins - 1
    return b


def hist_state(lo, hi, nbins):
    """One pore particle per value pair (vx = vy = 0, dx = vals[i], dy = vals[::-1][i]) that hits the z = 0 wall in the
    next step: the completed path carries px = |dx| and py = |dy| unchanged (Pore:274-278)."""
    p, c = _pore()
    p.hist_lo, p.hist_hi, p.hist_bins = float(lo), float(hi), int(nbins)
    s = EdgeState(p, c["dt"])
    vals = hist_values(lo, hi, nbins)
    n = len(vals)
    side = int(np.ceil(np.sqrt(n)))
    for i, (a, b) in enumerate(zip(vals, vals[::-1])):
        x = -2.0e-8 + 4.0e-8 * (i % side) / side
        y = -2.0e-8 + 4.0e-8 * (i // side) / side
        s.add("hist_value", x, y, -1.0e-11 - 1.0e-14 * i, 0.0, 0.0, -300.0, d=5.0e-8, dx=a, dy=b, dz=1.0e-9,
              flag=1, landed=False)
    s.extra["values"] = vals
    return s.finish()


# ---------------------------------------------------------------------------------------------------------- field bins
def field_positions(edges_r, edges_z):
    """axisymmetric positions: r exactly on every edge (x = r, y = 0 and +-0.0 mixes), r == 0, r == hi, r just above hi,
    z on every edge, on hi and just above; returns (x, y, z, cases)"""
    xs, ys, zs, cases = [], [], [], {}

    def put(name, x, y, z):
        cases.setdefault(name, []).append(len(xs))
        xs.append(x); ys.append(y); zs.append(z)

    zmid = 0.5 * (edges_z[0] + edges_z[1])
    rmid = 0.5 * (edges_r[0] + edges_r[1])
    for e in edges_r:
        put("r_edge", float(e), 0.0, zmid)
        put("r_edge", 0.0, -float(e), zmid)
    put("r_hi", float(edges_r[-1]), 0.0, zmid)
    put("r_beyond", float(np.nextafter(edges_r[-1], np.inf)), 0.0, zmid)
    for x, y in ((0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0)):
        put("r_zero", x, y, zmid)
    for e in edges_z:
        for zv in around(e, 1):
            put("z_edge", rmid, 0.0, zv)
    put("z_hi", rmid, 0.0, float(edges_z[-1]))
    put("z_beyond", rmid, 0.0, float(np.nextafter(edges_z[-1], np.inf)))
    return np.array(xs), np.array(ys), np.array(zs), cases


# ---------------------------------------------------------------------------------------------------------- energised walls
TEMP_SLOTS = 140      # azimuth slots of a ring: 1.34 nm of arc at R_p_c, more than three collision ranges


def _temp():
    return PR.pore_params(n=0, energised=True)


def _unit(k):
    """the unit vector of azimuth slot k; slots 0, 35, 70, 105 are the four axes, exactly"""
    q = k % TEMP_SLOTS
    if q % (TEMP_SLOTS // 4) == 0:
        return [(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)][q // (TEMP_SLOTS // 4)]
    a = 2.0 * np.pi * q / TEMP_SLOTS
    return float(np.cos(a)), float(np.sin(a))


def radius_side(Rsq, c, s, want):
    """(x, y) at sqrt(Rsq) * (c, s), the larger coordinate moved by up to 6 ulp so that x*x + y*y is "below", "on" or
    "above" Rsq by as little as doubles allow (the search of pore_bounds()); None if no such value is among them"""
    r0 = np.sqrt(np.float64(Rsq))
    x, y = float(r0 * c), float(r0 * s)
    major_x = abs(c) >= abs(s)
    best = None
    for v in around(x if major_x else y, 6):
        xx, yy = (v, y) if major_x else (x, v)
        q = xx * xx + yy * yy
        side = "on" if q == Rsq else ("above" if q > Rsq else "below")
        if side == want and (best is None or abs(q - Rsq) < best[0]):
            best = (abs(q - Rsq), xx, yy)
    return None if best is None else (best[1], best[2])


class _Slots:
    """azimuth slots per (zone, band): a zone is a z level, a band a radius; two particles of one zone and band never
    share a slot, and a fast particle takes two"""

    def __init__(self):
        self.cursor, self.axes = {}, {}

    def take(self, key, axis=False, wide=False):
        if axis:
            k = self.axes.get(key, 0)
            assert k < 4, key
            self.axes[key] = k + 1
            return k * (TEMP_SLOTS // 4)
        k = self.cursor.get(key, 1)
        if wide:
            k += 1
        while k % (TEMP_SLOTS // 4) == 0 or (wide and (k + 1) % (TEMP_SLOTS // 4) == 0):
            k += 1
        self.cursor[key] = k + (2 if wide else 1)
        assert self.cursor[key] <= TEMP_SLOTS, key
        return k


def temp_walls(reference_safe=False, far=True):
    """Particles on every plane and squared radius the energised wall sequence compares against (Temp:708-751, case ids
    3..9 in evaluation order), and at the corners where one particle is hit by two cases in one step.

    Zones are z levels (the four planes t_z3_hot, t_zgap_lo, t_zgap_hi, t_z3_cold and levels inside the hot coating, the
    gap and the cold coating), bands are radii (A: over the coatings / mid annulus, B: at R_p_c .. R_p, C: at R_g_c); every
    particle has an azimuth slot of its own in its zone and band.

    cases: ``cur_z_case<k>`` / ``prior_z_case<k>`` (z on a plane of case k and +-1, +-2 ulp, landed / uploaded),
    ``far_prior_case6|7`` (prior z on the OTHER gap plane), ``cur_r_<R>_case<k>_<side>`` / ``prior_r_<R>_case<k>_<side>``
    (x*x + y*y below / on / above a squared radius), ``corner_4_8``, ``corner_3_9``, ``corner_5_6``, ``corner_5_7``,
    ``prior_on_Rpc_6_8``, ``prior_on_Rpc_7_9``, ``vz0_on_plane`` and, unless reference_safe, ``tiny_vx_plane``.
    There is no corner_7_9 of its own: case 7 wants a prior radius^2 >= R_p_c_sq and case 9 one <= R_p_c_sq, so the pair
    can only meet on a prior radius^2 == R_p_c_sq, which is prior_on_Rpc_7_9.

    far=False leaves out far_prior_case6|7: 160 km/s, a momentum change beyond the range of the sampled surfaces' quantisers.
    reference_safe drops what the reference cannot execute under np.seterr(all='raise'): a plane hit whose vx**2
    underflows (hit_vertical_coated_wall has no try block)."""
    p, c = _temp()
    dt = c["dt"]
    s = EdgeState(p, dt)
    slots = _Slots()
    zc, zh, zlo, zhi = p.t_z3_cold, p.t_z3_hot, p.t_zgap_lo, p.t_zgap_hi
    v, vfast = 431.0, 2600.0
    hop, step = v * dt, vfast * dt
    R_out, R_ann = p.R_p + 2.0e-9, 0.5 * (p.R_p_c + p.R_g_c)

    def put(case, key, z, vr, vt, vz, landed, r=None, side=None, axis=False, wide=False, tries=1, jitter=True):
        """one particle of `case` in the next free slot of `key`: at radius r, or on `side` = (Rsq, want) of a squared
        radius; the velocity is vr along the radius and vt across it.  flag alternates within the case."""
        for _ in range(tries):
            k = slots.take(key, axis=axis, wide=wide)
            cs, sn = _unit(k)
            xy = (r * cs, r * sn) if side is None else radius_side(side[0], cs, sn, side[1])
            if xy is None:
                if axis:
                    return None
                continue
            i = s.add(case, xy[0], xy[1], z, vr * cs - vt * sn, vr * sn + vt * cs, vz, flag=len(s.cases.get(case, [])) % 2,
                      landed=landed, jitter=jitter)
            if i is not None:
                return i
        return None

    # ---- planes: z on the plane and next to it, current (landed) and prior (uploaded), both signs of vz
    planes = {3: (zc, "cold_mouth", R_out), 4: (zh, "hot_mouth", R_out), 6: (zlo, "gap_lo", R_ann), 7: (zhi, "gap_hi", R_ann)}
    for k, (zp, zone, r) in planes.items():
        for zv in around(zp):
            for vz in (-v, v):
                assert put(f"cur_z_case{k}", (zone, "A"), zv, 97.0, -61.0, vz, True, r=r, tries=3) is not None
                put(f"prior_z_case{k}", (zone, "A"), zv, 97.0, -61.0, vz, False, r=r)
        for vz in (0.0, -0.0):
            put("vz0_on_plane", (zone, "A"), zp, 97.0, -61.0, vz, False, r=r)
        if not reference_safe:
            vz = -v if k in (3, 6) else v
            put("tiny_vx_plane", (zone, "A"), zp + 0.5 * dt * vz, 3.0 * TINY, 0.0, vz, True, r=r, axis=True, jitter=False)
    # prior z on the OTHER gap plane: through the whole gap in one step (pz <= t_zgap_hi in case 6, pz >= t_zgap_lo in case 7)
    span = zhi - zlo
    for zv in around(zhi) if far else ():
        put("far_prior_case6", ("gap_hi", "A"), zv, 97.0, -61.0, -(span + 0.5 * hop) / dt, False, r=R_ann)
    for zv in around(zlo) if far else ():
        put("far_prior_case7", ("gap_lo", "A"), zv, 97.0, -61.0, (span + 0.5 * hop) / dt, False, r=R_ann)
    # case 5's strict pz > t_zgap_lo, pz < t_zgap_hi: leaving the annulus across R_g_c with the prior z on a gap plane
    for zp, zone, sgn in ((zlo, "gap_lo", 1.0), (zhi, "gap_hi", -1.0)):
        for zv in around(zp):
            for vz in (40.0 * sgn, -40.0 * sgn):
                put("prior_z_case5", (zone, "C"), zv, v, -61.0, vz, False, r=p.R_g_c - 0.4 * hop)
    # crossing R_p_c with the current z on a plane: closed ends in case 8 (>= t_z3_hot, <= t_zgap_lo), open in case 9
    for zp, zone, k in ((zh, "hot_mouth", 8), (zlo, "gap_lo", 8), (zhi, "gap_hi", 9), (zc, "cold_mouth", 9)):
        for zv in around(zp, 1):
            for vz in (-40.0, 40.0, 0.0):
                if zv != zp and vz == 0.0:
                    continue
                put(f"cur_z_case{k}", (zone, "B"), zv, v, -61.0, vz, True, r=p.R_p_c + 0.5 * hop, tries=3)
    # ---- squared radii: below / on / above, on an axis and at an oblique azimuth
    def radii(name, key, Rsq, z, vr, vz, landed):
        for want in ("below", "on", "above"):
            for axis in (True, False):
                put(f"{name}_{want}", key, z, vr, -61.0, vz, landed, side=(Rsq, want), axis=axis, tries=1 if axis else 40)

    radii("cur_r_Rp_case4", ("hot_mouth", "B"), p.R_p_sq, zh + 0.5 * hop, 97.0, v, True)
    radii("cur_r_Rp_case3", ("cold_mouth", "B"), p.R_p_sq, zc - 0.5 * hop, 97.0, -v, True)
    radii("cur_r_Rgc_case5", ("gap_140", "C"), p.R_g_c_sq, 140.0e-9, v, 40.0, True)
    radii("prior_r_Rgc_case5", ("gap_150", "C"), p.R_g_c_sq, 150.0e-9, v, 40.0, False)
    radii("cur_r_Rpc_case8", ("hot_110", "B"), p.R_p_c_sq, 110.0e-9, v, 40.0, True)
    radii("cur_r_Rpc_case9", ("cold_200", "B"), p.R_p_c_sq, 200.0e-9, v, 40.0, True)
    radii("prior_r_Rpc_case8", ("hot_118", "B"), p.R_p_c_sq, 118.0e-9, v, 40.0, False)
    radii("prior_r_Rpc_case9", ("cold_210", "B"), p.R_p_c_sq, 210.0e-9, v, 40.0, False)
    radii("prior_r_Rpc_case6", ("gap_lo", "B"), p.R_p_c_sq, zlo + 0.5 * hop, 97.0, -v, False)
    radii("prior_r_Rpc_case7", ("gap_hi", "B"), p.R_p_c_sq, zhi - 0.5 * hop, 97.0, v, False)
    # ---- corners: two cases on one particle in one step (fast particles, uploaded), each at its own azimuth
    for q in range(12):
        f, g = 0.06 + 0.04 * q, 0.25 + 0.05 * q
        # up and outward past the hot mouth: case 4 parks it on t_z3_hot, case 8's z >= t_z3_hot then holds
        put("corner_4_8", ("hot_mouth", "B"), zh - g * step, vfast, 0.0, vfast, False, r=p.R_p_c - f * step, wide=True)
    # the same with a radial speed that puts the contact with the plane 2 nm outside R_p_c: case 8's solve, on the redrawn
    # velocity, then misses the cylinder for a fifth of the directions (slots 100 .. 133 of bands A and B, kept free)
    assert max(slots.cursor[("hot_mouth", "A")], slots.cursor[("hot_mouth", "B")]) <= 99
    for q in range(12):
        cs, sn = _unit(100 + 3 * q)
        r0, vr = p.R_p_c - 0.02e-9 * (q + 1), 1.15e4        # (11.5 km/s: its energy is still inside the sampled surfaces' range)
        s.add("corner_4_8", r0 * cs, r0 * sn, zh - 0.9 * step, vr * cs, vr * sn, vfast, flag=q % 2, landed=False)
    for q in range(8):        # (eight of each: the reference's own initialisation needs 268 particles or more to populate every region)
        f, g = 0.06 + 0.08 * q, 0.2 + 0.1 * q
        # the mirrored cold mouth: case 3 parks it on t_z3_cold, case 9 asks z < t_z3_cold
        put("corner_3_9", ("cold_mouth", "B"), zc + g * step, vfast, 0.0, -vfast, False, r=p.R_p_c - f * step, wide=True)
        # out of the gap annulus across R_g_c and a gap plane: the plane is crossed first, so case 5's contact lies beyond it
        f = 0.2 + 0.1 * q
        put("corner_5_6", ("gap_lo", "C"), zlo + 0.5 * f * step, vfast, 0.0, -vfast, False, r=p.R_g_c - f * step, wide=True)
        put("corner_5_7", ("gap_hi", "C"), zhi - 0.5 * f * step, vfast, 0.0, vfast, False, r=p.R_g_c - f * step, wide=True)
        # prior radius^2 == R_p_c_sq: both r02 >= (cases 6, 7) and r02 <= (cases 8, 9) hold
        put("prior_on_Rpc_6_8", ("gap_lo", "B"), zlo + f * step, vfast, 0.0, -vfast, False, side=(p.R_p_c_sq, "on"), wide=True,
            tries=20)
        put("prior_on_Rpc_7_9", ("gap_hi", "B"), zhi - f * step, vfast, 0.0, vfast, False, side=(p.R_p_c_sq, "on"), wide=True,
            tries=20)
    return s.finish()


def temp_many_hits(n=2700):
    """A few thousand particles that all cross coated planes in the first step: more hits in that one step than the device
    sums' tile holds (2048), fewer than the record capacity (4096) in any one case, spread over cases 3, 4, 6, 7 and 8.
    The kinds are interleaved by particle index, so that no case's records arrive in index order.  Case 8 is hit only by
    corner_4_8-style particles, after case 4 has redrawn their velocity: whether its solve has a real root depends on the
    drawn direction, so some of them fail and some do not.  Case 9 is hit by five overflowing particles only: every one of
    its hits is a failed solve."""
    p, c = _temp()
    dt = c["dt"]
    s = EdgeState(p, dt)
    zc, zh, zlo, zhi = p.t_z3_cold, p.t_z3_hot, p.t_zgap_lo, p.t_zgap_hi
    v, vfast = 431.0, 2600.0
    hop, step = v * dt, vfast * dt
    third = n // 3
    # over the coatings at the two mouths: a square grid, 1.3 nm
    g = np.arange(-62.0e-9, 62.0e-9, 1.3e-9)
    X, Y = np.meshgrid(g, g, indexing="ij")
    R = np.hypot(X, Y)
    keep = (R > p.R_p + 1.6e-9) & (R < 60.0e-9)
    order = np.argsort(R[keep], kind="stable")
    grid = list(zip(X[keep][order].tolist(), Y[keep][order].tolist()))
    assert len(grid) >= third
    k3 = [("many_case3", x, y, zc + 0.4 * hop, 30.0 + 0.01 * j, -20.0 - 0.02 * j, -(v + 0.37 * j)) for j, (x, y) in enumerate(grid[:third])]
    k4 = [("many_case4", x, y, zh - 0.4 * hop, -25.0 - 0.01 * j, 35.0 + 0.02 * j, v + 0.41 * j) for j, (x, y) in enumerate(grid[:third])]
    # the corner of the hot mouth (cases 4 and 8) and the two bases of the gap annulus (cases 6, 7), on rings
    n48 = 130
    a48 = []
    for j in range(n48):
        cs, sn = float(np.cos(2.0 * np.pi * j / TEMP_SLOTS)), float(np.sin(2.0 * np.pi * j / TEMP_SLOTS))
        f, gz = 0.06 + 0.003 * j, 0.25 + 0.004 * j
        r0 = p.R_p_c - f * step
        a48.append(("many_corner_4_8", r0 * cs, r0 * sn, zh - gz * step, vfast * cs, vfast * sn, vfast))
    per = (n - 2 * third - n48 + 1) // 2
    k6, k7 = [], []
    rings = (p.R_p_c + 0.6e-9, p.R_p_c + 1.9e-9, p.R_p_c + 3.2e-9)
    for j in range(per):
        a = 2.0 * np.pi * (j % TEMP_SLOTS + 0.5 * ((j // TEMP_SLOTS) % 2)) / TEMP_SLOTS     # (staggered from ring to ring)
        cs, sn = float(np.cos(a)), float(np.sin(a))
        r = rings[j // TEMP_SLOTS]
        k6.append(("many_case6", r * cs, r * sn, zlo + 0.4 * hop, 20.0 + 0.03 * j, -15.0, -(v + 0.29 * j)))
        k7.append(("many_case7", r * cs, r * sn, zhi - 0.4 * hop, -20.0 - 0.03 * j, 15.0, v + 0.31 * j))
    rest, streams = [], [a48, k6, k7]
    while any(streams):
        for st in streams:
            if st:
                rest.append(st.pop(0))
    rest = rest[:n - 2 * third]
    for i in range(n):
        src = (k3, k4, rest)[i % 3]
        case, x, y, z, vx, vy, vz = src[i // 3]
        s.add(case, x, y, z, vx, vy, vz, flag=(i // 3) % 2, landed=False, jitter=False)
    for k in range(5):                  # case 9: every hit a failed solve
        _overflowing(s, "many_failed_case9", 204.0e-9 + 5.0e-9 * k, k)
    return s.finish()


DRAW_PER_CASE, DRAW_LADDER, DRAW_CORNERS = 190, 95, 8


def draw_ladder_z(p):
    """The contact z values of temp_draw_hits()'s ladder: next to either gap plane (1 and 3 ulp inside), the midpoint, the
    rest evenly spaced across the gap."""
    zlo, zhi = np.float64(p.t_zgap_lo), np.float64(p.t_zgap_hi)
    lo1, hi1 = np.nextafter(zlo, np.inf), np.nextafter(zhi, -np.inf)
    lo3, hi3 = np.nextafter(np.nextafter(lo1, np.inf), np.inf), np.nextafter(np.nextafter(hi1, -np.inf), -np.inf)
    rest = np.linspace(zlo, zhi, DRAW_LADDER - 4 + 2)[1:-1]          # (an odd number of them: the middle one is the midpoint)
    rest[len(rest) // 2] = 0.5 * (zlo + zhi)
    zs = [lo1, lo3, hi1, hi3] + rest.tolist()
    assert len(zs) == DRAW_LADDER and len(set(float(z) for z in zs)) == DRAW_LADDER
    return [float(z) for z in zs]


def temp_draw_hits():
    """About 1,350 particles, every one hit by exactly one case in the first step — 190 per case, ``draw_case<k>`` — but for
    eight ``draw_corner_4_8`` particles, which case 4 parks on t_z3_hot and case 8 takes next: two draws in one step under
    two case words.  It is there for the device draws (tests/test_gpu_draws.py): many hits of every case whatever the step
    word is, normals all round the circle, and gap hits at chosen heights.

    The plane cases (3, 4 over the coatings at the mouths, 6, 7 on the bases of the gap annulus) stand on the grids of
    temp_many_hits(); their normals are (0, 0, +-1) exactly.  The cylinder cases (5 at R_g_c, 8 and 9 at R_p_c) go round the
    azimuth slots — the first 140 of a case on the slots themselves, the four exact axes included (there without a
    tangential velocity, so that the normal lies on the axis), the other 50 half a slot on.  The first 95 of case 5 are the
    ``draw_ladder``: vz = 0, so the contact z is the uploaded z bit for bit (draw_ladder_z()).  Kinds are interleaved by
    particle index and flags alternate within a kind.  No particle overflows."""
    p, c = _temp()
    dt = c["dt"]
    s = EdgeState(p, dt)
    zc, zh, zlo, zhi = p.t_z3_cold, p.t_z3_hot, p.t_zgap_lo, p.t_zgap_hi
    v, vfast = 431.0, 2600.0
    hop, step = v * dt, vfast * dt
    n = DRAW_PER_CASE
    g = np.arange(-62.0e-9, 62.0e-9, 1.3e-9)
    X, Y = np.meshgrid(g, g, indexing="ij")
    R = np.hypot(X, Y)
    keep = (R > p.R_p + 1.6e-9) & (R < 60.0e-9)
    order = np.argsort(R[keep], kind="stable")
    grid = list(zip(X[keep][order].tolist(), Y[keep][order].tolist()))[:n]
    k3 = [("draw_case3", x, y, zc + 0.4 * hop, 30.0 + 0.01 * j, -20.0 - 0.02 * j, -(v + 0.37 * j)) for j, (x, y) in enumerate(grid)]
    k4 = [("draw_case4", x, y, zh - 0.4 * hop, -25.0 - 0.01 * j, 35.0 + 0.02 * j, v + 0.41 * j) for j, (x, y) in enumerate(grid)]

    def ring(j):
        """(cos, sin, on an exact axis) of the j-th particle of a ring"""
        if j < TEMP_SLOTS:
            cs, sn = _unit(j)
            return cs, sn, j % (TEMP_SLOTS // 4) == 0
        a = 2.0 * np.pi * (j - TEMP_SLOTS + 0.5) / TEMP_SLOTS
        return float(np.cos(a)), float(np.sin(a)), False

    k6, k7 = [], []
    for j in range(n):
        cs, sn, _ = ring(j)
        r = p.R_p_c + (0.6e-9 if j < TEMP_SLOTS else 1.9e-9)
        k6.append(("draw_case6", r * cs, r * sn, zlo + 0.4 * hop, 20.0 + 0.03 * j, -15.0, -(v + 0.29 * j)))
        k7.append(("draw_case7", r * cs, r * sn, zhi - 0.4 * hop, -20.0 - 0.03 * j, 15.0, v + 0.31 * j))

    def cylinder(name, Rc, zs, vzs):
        out = []
        for j in range(n):
            cs, sn, axis = ring(j)
            vr, vt = v + 0.3 * j, 0.0 if axis else -61.0
            r0 = Rc - 0.4 * hop
            out.append((name(j), r0 * cs, r0 * sn, zs[j], vr * cs - vt * sn, vr * sn + vt * cs, vzs[j]))
        return out

    ladder = draw_ladder_z(p)
    span = zhi - zlo
    z5 = ladder + [zlo + span * (0.07 + 0.86 * (j / (n - DRAW_LADDER))) for j in range(n - DRAW_LADDER)]
    vz5 = [0.0] * DRAW_LADDER + [40.0 if j % 2 else -40.0 for j in range(n - DRAW_LADDER)]
    k5 = cylinder(lambda j: "draw_ladder" if j < DRAW_LADDER else "draw_case5", p.R_g_c, z5, vz5)
    k8 = cylinder(lambda j: "draw_case8", p.R_p_c, [110.0e-9 if j < TEMP_SLOTS else 118.0e-9 for j in range(n)],
                  [40.0 if j % 2 else -40.0 for j in range(n)])
    k9 = cylinder(lambda j: "draw_case9", p.R_p_c, [200.0e-9 if j < TEMP_SLOTS else 210.0e-9 for j in range(n)],
                  [-40.0 if j % 2 else 40.0 for j in range(n)])
    a48 = []
    for j in range(DRAW_CORNERS):
        cs, sn = _unit(3 + 17 * j)
        f, gz = 0.06 + 0.04 * j, 0.25 + 0.05 * j
        r0 = p.R_p_c - f * step
        a48.append(("draw_corner_4_8", r0 * cs, r0 * sn, zh - gz * step, vfast * cs, vfast * sn, vfast))
    streams = [k3, k5, k4, k8, k6, k9, k7, a48]
    count = {}
    while any(streams):
        for st in streams:
            if st:
                case, x, y, z, vx, vy, vz = st.pop(0)
                s.add(case, x, y, z, vx, vy, vz, flag=count.get(case, 0) % 2, landed=False, jitter=False)
                count[case] = count.get(case, 0) + 1
    return s.finish()


def assert_temp_coverage(s, masks, failed):
    """What a run of temp_walls() must have exercised in its first step, whoever ran it (the reference in the fixture, the
    oracle beside the GPU): ``masks[case]`` = the particle indices hit by case 3 .. 9, ``failed`` = the number of contact
    solves without a real root."""
    m = {k: set(int(i) for i in masks[k]) for k in range(3, 10)}
    assert all(len(m[k]) > 0 for k in m), {k: len(v) for k, v in m.items()}
    corner = {k: set(s.cases[k]) for k in ("corner_4_8", "corner_3_9", "corner_5_6", "corner_5_7", "prior_on_Rpc_6_8",
                                          "prior_on_Rpc_7_9")}
    assert len(corner["corner_4_8"] & m[4] & m[8]) >= 6                  # parked on t_z3_hot by case 4, taken by case 8's z >= t_z3_hot
    assert len(corner["corner_5_6"] & m[5] & m[6]) >= 6 and len(corner["corner_5_7"] & m[5] & m[7]) >= 6
    on = corner["prior_on_Rpc_6_8"] | corner["prior_on_Rpc_7_9"]
    assert all(s.x[i] * s.x[i] + s.y[i] * s.y[i] == s.p.R_p_c_sq for i in on)
    assert len(corner["prior_on_Rpc_6_8"] & m[6] & m[8]) >= 6            # r02 >= R_p_c_sq and r02 <= R_p_c_sq both hold
    assert corner["corner_3_9"] <= m[3] and not corner["corner_3_9"] & m[9]          # z == t_z3_cold is not < t_z3_cold
    assert corner["prior_on_Rpc_7_9"] <= m[7] and not corner["prior_on_Rpc_7_9"] & m[9]      # z == t_zgap_hi is not > t_zgap_hi
    assert failed >= 1


def _overflowing(s, name, z, k):
    """A particle whose cylinder solve fails for certain: vx = 1e155 carries it from inside the pore far beyond every radius
    (x*x stays finite) and makes a = vx*vx infinite, so b*b - 4*a*c is inf - inf.  The open-air wall's specular solve fails the
    same way first (counted, particle left alone), then case 8 or 9 by its z; the bounds check takes the particle back to the
    axis.  Not for the reference: it raises on the overflow."""
    s.add(name, 1.0e-9 + 0.1e-9 * k, 0.0, z, 1.0e155, 0.0, 0.0, flag=k % 2, landed=False, jitter=False)


def temp_failed_only():
    """One step in which the hot sum's only hits are failed solves (case 8, overflowing) while the cold sum has good hits
    (case 3) and failed ones (case 9): the device sums fold + 0.0 for case 8 and leave the hot flag clear."""
    p, c = _temp()
    s = EdgeState(p, c["dt"])
    hop = 431.0 * c["dt"]
    for k in range(5):
        _overflowing(s, "only_failed_case8", 104.0e-9 + 5.0e-9 * k, k)
        _overflowing(s, "only_failed_case9", 204.0e-9 + 5.0e-9 * k, k)
        cs, sn = _unit(7 * k + 1)
        s.add("good_case3", (p.R_p + 2.0e-9) * cs, (p.R_p + 2.0e-9) * sn, p.t_z3_cold + 0.4 * hop, 30.0, -20.0, -431.0 - k, flag=k % 2,
              landed=False)
    return s.finish()
