"""Crafted movers, each at one limit written into the kept per-cell lists (amc_list_keep, amc_grid_dev.h; the cycle:
amc_list_build_mode, amc_stream.hip): the fence idx == wave_cap - 1, a wave whose 64 lanes all move in one step, lane 63's
ballot mask, the last and partial wave, a dead and a live node of one particle in one list, a pair that exists only between
pool nodes, a mover that takes its state from the lazy commit, a jump by the bounds check, the pore's narrow layer windows.

Pure NumPy and deterministic (no random numbers).  Lengths are in grid cells (h) along the marching axis and in collision
ranges (cr) between partners.  ``t`` counts steps from 0: step t of a cycle of K is a full build when t % K == 0 and a step in
between otherwise; a state runs for 2 K + 1 steps (``steps(K)``): two whole cycles and the full build of a third.

The grid: ``grid_of`` restates setup_grid (amc_api.hip) — faces at xlo - h + k h, the cell enlarged by 1.26 until the full
table stays below 2e8 cells (the pore at both cell sizes asked for here: the catalogue takes the h the library ends up
with), per-layer windows in the pore.  ``filed_cell`` restates amc_list_keep's cell: the position relative to the grid
origin rounded to single precision, the origin added back, amc_grid_coords, amc_grid_cell.  ``movers_per_wave`` turns the
positions after each step's streaming stages into the counter every wave (index // 64) must show.

Marchers drift exactly 1.0 h per step along one axis, mid-cell (or a fixed fraction of a cell) in the others: every step takes
them across exactly one face and their list node comes from the wave's pool.  Resters creep (1e-3 cr per step) and stay in
the cell of the full build.  Index layout (before the permutation): waves 0-2 the three full marching waves (+x, -y, +z),
waves 3-5 resting waves with movers in single lanes, waves 6-11 resters with the partners of the pair cases spread over them,
then a partial wave of 37 whose last three march.  ``reversed`` mirrors the indices of the whole waves (wave w -> 11 - w,
lane l -> 63 - l) and leaves the partial wave in place; the cases whose point is a lane are pinned to their final lane.

Distance rule (as tests/cluster_states.py): after a streaming pass no two particles are 0.9 to 1.1 cr apart; and no particle
is within 1e-3 h of a grid face, in any step, hit or not — except in ``face_rounding``, which is about that and is a state of
its own.  That is why every pair meets on ONE line, its marching axis, with a partner that creeps along that axis only: equal
masses exchange their velocities along the line, so a marcher that has hit rests and a rester that was hit marches on, at
the same known fractions of a cell in the other two axes."""
from __future__ import annotations

import numpy as np

from argon_monte_carlo_amd import params as PR
from tests.edge_states import STATE, EdgeState, around

KINDS = ("cube", "pore")
PERMS = ("identity", "reversed")
CELLS = ("min", "wide")             # fine_cell: the smallest the library takes (edge_states.grid_pairs), 3.3 cr
KS = (2, 3, 4, 8)
FULL_WAVES, LANE_WAVES, MIXED_WAVES, TAIL, TAIL_MARCHERS = 3, 3, 6, 37, 3
WAVES = FULL_WAVES + LANE_WAVES + MIXED_WAVES
N_MAIN = 64 * WAVES
FULL_DIRS = ((0, 1.0), (1, -1.0), (2, 1.0))          # (axis, sign) of full wave 0, 1, 2: the new cell id larger, smaller, larger


def steps(K):
    return 2 * K + 1


def _params(kind):
    if kind == "cube":
        return PR.cube_params(n=0, cube_side=100.0e-9, n_sub=5)
    return PR.pore_params(n=0, energised=(kind == "temp"))       # ("temp": the energised pore, the same geometry)


def fine_cell(p, cell):
    return (2.01 * 1.02 if cell == "min" else 3.3) * p.collision_range


# ---------------------------------------------------------------------------------------------------------------- host mirror
class Grid:
    pass


def grid_of(p, h):
    """setup_grid (amc_api.hip) for params p and a requested fine_cell h > 0, in the same double arithmetic"""
    cr = p.collision_range
    G = Grid()
    G.uniform = p.geometry == 1
    if G.uniform:
        xlo, xhi, zlo, zhi = 0.0, max(p.cube_x, p.cube_y), 0.0, p.cube_z
    else:
        xlo, xhi, zlo, zhi = -p.R_oa, p.R_oa, 0.0, p.H
    h = float(h)
    while True:
        nxy, nz = np.ceil((xhi - xlo) / h) + 2, np.ceil((zhi - zlo) / h) + 2
        if nxy * nxy * nz < 2.0e8:
            break
        h *= 1.26
    G.h, G.inv_h = h, 1.0 / h
    G.x0 = G.y0 = xlo - h
    G.z0 = zlo - h
    G.gx = G.gy = int(np.ceil((xhi - xlo) / h)) + 2
    G.gz = int(np.ceil((zhi - zlo) / h)) + 2
    G.lay_lo = np.zeros(G.gz, dtype=np.int64)
    G.lay_n = np.full(G.gz, G.gx, dtype=np.int64)
    if not G.uniform:
        body_lo, body_hi = p.h_oa + h + cr, p.z_cold - h - cr
        w_lo = max(0, int(np.floor((-p.R_g - cr - G.x0) / h)) - 1)
        w_hi = min(G.gx - 1, int(np.floor((p.R_g + cr - G.x0) / h)) + 1)
        z_a = G.z0 + np.arange(G.gz) * h
        body = (z_a > body_lo) & (z_a + h < body_hi)
        G.lay_lo[body], G.lay_n[body] = w_lo, w_hi - w_lo + 1
    G.lay_off = np.concatenate([[0], np.cumsum(G.lay_n * G.lay_n)[:-1]])
    G.ncells = int((G.lay_n * G.lay_n).sum())
    return G


def grid_coords(G, x, y, z):
    """amc_list_keep's coordinates: of the single-precision record, read back as amc_rec_pos does"""
    out = []
    for v, o, g in ((x, G.x0, G.gx), (y, G.y0, G.gy), (z, G.z0, G.gz)):
        r = (np.asarray(v, dtype=np.float64) - o).astype(np.float32).astype(np.float64)
        back = o + r
        out.append(np.clip(np.floor((back - o) * G.inv_h), 0, g - 1).astype(np.int64))
    return out


def grid_cell(G, cx, cy, cz):
    """amc_grid_cell: (cell id, outside)"""
    if G.uniform:
        return (cz * G.gy + cy) * G.gx + cx, np.zeros(np.shape(cx), dtype=bool)
    lo, n = G.lay_lo[cz], G.lay_n[cz]
    lx, ly = cx - lo, cy - lo
    outside = (lx < 0) | (lx >= n) | (ly < 0) | (ly >= n)
    lx, ly = np.clip(lx, 0, n - 1), np.clip(ly, 0, n - 1)
    return G.lay_off[cz] + ly * n + lx, outside


def filed_cell(p, h, x, y, z):
    """the cell the kept lists file a particle at (x, y, z) under, and whether it was clamped into its layer's window"""
    G = grid_of(p, h)
    return grid_cell(G, *grid_coords(G, x, y, z))


def movers_per_wave(p, h, pre, K, wave=None, nwaves=None):
    """pre[t] = (x, y, z) after the streaming stages of step t, before the sweep.  Returns (count[t, wave], outside[t]):
    what every wave has handed out of its pool after step t — zero after a full build (t % K == 0), else what it had plus
    the particles filed under another cell than one step before.  wave: the wave of every particle (default index // 64)."""
    G = grid_of(p, h)
    n = np.shape(pre[0][0])[0]
    wave = np.arange(n) // 64 if wave is None else np.asarray(wave)
    nwaves = int(wave.max()) + 1 if nwaves is None else nwaves
    counts = np.zeros((len(pre), nwaves), dtype=np.int64)
    outside = np.zeros(len(pre), dtype=bool)
    cell_of = None
    for t, (x, y, z) in enumerate(pre):
        c, out = grid_cell(G, *grid_coords(G, x, y, z))
        outside[t] = out.any()
        if t % K:
            counts[t] = counts[t - 1] + np.bincount(wave[c != cell_of], minlength=nwaves)
        cell_of = c
    return counts, outside


def exchange_waves(n, world, rank):
    """The wave that files particle p on `rank` of a sharded run (amc_exchange.hip): its own shard by the pack kernel, 64
    consecutive particles of the shard per wave; the others by the unpack kernel, behind the pack's waves, every shard in a
    block of `per` slots.  Returns (wave[p], number of waves)."""
    m = max((n + world - 1) // world, 1)
    cap = (max(4096, m // 8) + 15) // 16 * 16
    per = max(m, cap)
    waves_pack, waves_unpack = (m + 255) // 256 * 4, (world * per + 255) // 256 * 4
    base, rem = n // world, n % world
    wave = np.empty(n, dtype=np.int64)
    for r in range(world):
        lo = r * base + min(r, rem)
        u = np.arange(base + (1 if r < rem else 0))
        wave[lo + u] = u // 64 if r == rank else waves_pack + (r * per + u) // 64
    return wave, waves_pack + waves_unpack


def expected_stats(counts, K):
    """what lists_stats() must show after step t: (lists_age, count_sum, count_max, full_builds)"""
    return [(t % K, int(counts[t].sum()), int(counts[t].max()), t // K + 1) for t in range(len(counts))]


# ---------------------------------------------------------------------------------------------------------------- the builder
def _fin(r, perm):
    """final index of layout row r"""
    return r if perm == "identity" or r >= N_MAIN else N_MAIN - 1 - r


class _Builder:
    def __init__(self, kind, perm, cell, K):
        self.kind, self.perm, self.K = kind, perm, K
        self.p, c = _params(kind)
        self.consts = c
        self.dt = c["dt"]
        self.cr = self.p.collision_range
        self.h_asked = fine_cell(self.p, cell)
        self.G = grid_of(self.p, self.h_asked)
        self.h = self.G.h
        self.u = self.cr / self.h                   # one collision range in cells
        self.spec = {}                              # final index -> (case, start position, velocity)
        self.meet, self.cells_of, self.waves = [], [], {}
        self._mixed = 0
        self._rows = iter(self._row_anchors())

    # -- coordinates: cell k, fraction f
    def at(self, k, f=(0.5, 0.5, 0.5)):
        o = np.array([self.G.x0, self.G.y0, self.G.z0])
        return o + (np.asarray(k, dtype=np.float64) + np.asarray(f, dtype=np.float64)) * self.h

    def cell_at(self, pos):
        o = np.array([self.G.x0, self.G.y0, self.G.z0])
        return np.floor((np.asarray(pos) - o) / self.h).astype(np.int64)

    def _row_anchors(self):
        """meeting cells of the pair cases: one row (y, z) each, 3 h either side of the middle of a reference cell, the
        meeting x in the middle of a reference cell; marchers come and go along x"""
        p = self.p
        if self.kind == "cube":
            xm, ycs, zcs = 1.5 * p.dx, [(k + 0.5) * p.dy for k in (2, 3, 4)], [(k + 0.5) * p.dz for k in range(5)]
        else:
            xm, ycs, zcs = 0.5 * p.dx, [(k + 0.5) * p.dy for k in (-2, -1, 0, 1)], [(k + 0.5) * p.dz for k in (0, 1, 2)]
        out = []
        for zc in zcs:
            for yc in ycs:
                for sy in (-3, 3):
                    for sz in (-3, 3):
                        out.append(self.cell_at([xm, yc + sy * self.h, zc + sz * self.h]))
        return out

    def row(self):
        return next(self._rows)

    # -- indices
    def mixed(self, m=1):
        """m layout rows in m different resting waves (6 ..), ascending"""
        out = []
        for _ in range(m):
            k = self._mixed
            self._mixed += 1
            out.append(64 * (FULL_WAVES + LANE_WAVES + k % MIXED_WAVES) + 3 + 2 * (k // MIXED_WAVES))
        return sorted(out)

    def ordered(self, m=2):
        """m final indices in different waves, ascending in the FINAL order whatever the permutation"""
        return sorted(_fin(r, self.perm) for r in self.mixed(m))

    def put(self, final, case, start, vel):
        assert final not in self.spec, (final, case)
        self.spec[int(final)] = (case, np.asarray(start, dtype=np.float64), np.asarray(vel, dtype=np.float64))
        return int(final)

    def marcher(self, final, case, pos, t, axis=0, sign=1.0, extra=(0.0, 0.0, 0.0)):
        """a particle that is at pos after the streaming stages of step t and drifts sign * 1.0 h per step along axis
        (plus `extra`, in metres per step)"""
        d = np.array(extra, dtype=np.float64)
        d[axis] += sign * self.h
        return self.put(final, case, np.asarray(pos) - (t + 1) * d, d / self.dt)

    def rester(self, final, case, pos, axis=None):
        """a particle at pos after step 0 that creeps on, 1e-3 cr per step or less.  axis: along that axis only — the partner
        of a marcher along it, so that the two meet on one line and stay on it afterwards"""
        k = len(self.spec)
        d = 1.0e-3 * self.cr * np.array([1 + k % 3, -1 - k % 5, 1 + k % 7]) / 7.0
        if axis is not None:
            d = d * np.eye(3)[axis]
        return self.put(final, case, np.asarray(pos) - d, d / self.dt)

    def finish(self, which, shift=0, pad=0):
        """shift / pad: resters in front of and behind the layout (sharded runs: where the shard boundaries fall); shift is a
        multiple of 64, so the layout's waves stay waves"""
        assert shift % 64 == 0
        n = N_MAIN + TAIL
        spots = iter(self._filler_spots())
        s = EdgeState(self.p, self.dt)
        for q in range(-shift, n + pad):
            if q not in self.spec:
                self.rester(q, "filler", next(spots))
            case, start, vel = self.spec[q]
            s.add(case, *start, *vel, flag=1, landed=False, jitter=False)       # (flag set: every hit leaves a record)
        s.finish()
        self.meet = [(c, i + shift, j + shift, t) for c, i, j, t in self.meet]
        self.cells_of = [(c, i + shift, cells) for c, i, cells in self.cells_of]
        self.waves = {k: (w + shift // 64, m) for k, (w, m) in self.waves.items()}
        s.p.fine_cell, s.p.detect_mode = self.h_asked, 1
        s.p.reserved1 = 1                   # (a failed wall solve is counted, not fatal: bounds_jump)
        s.extra.update(kind=self.kind, perm=self.perm, K=self.K, h=self.h, h_asked=self.h_asked, which=which, consts=self.consts,
                       meet=list(self.meet), cells_of=list(self.cells_of), waves=dict(self.waves))
        return s

    def _filler_spots(self):
        nm = 1.0e-9
        if self.kind == "cube":
            lo, hi = [68 * nm, 34 * nm, 34 * nm], [94 * nm, 66 * nm, 94 * nm]
        else:
            lo, hi = [45 * nm, -40 * nm, 10 * nm], [100 * nm, 40 * nm, 90 * nm]
        k0, k1 = self.cell_at(lo), self.cell_at(hi)
        return [self.at([kx, ky, kz]) for kz in range(k0[2], k1[2], 3) for ky in range(k0[1], k1[1], 3)
                for kx in range(k0[0], k1[0], 3)]


# ---------------------------------------------------------------------------------------------------------------- the cases
def _march_full(b):
    """three whole waves: an 8 x 8 array two cells apart across the marching axis, every particle mid-cell"""
    nm = 1.0e-9
    corner = {"cube": ([8 * nm, 5 * nm, 5 * nm], [70 * nm, 95 * nm, 5 * nm], [70 * nm, 5 * nm, 5 * nm]),
              "pore": ([-110 * nm, -11 * nm, 20 * nm], [-70 * nm, 40 * nm, 20 * nm], [-70 * nm, -40 * nm, 20 * nm])}
    corner = corner["cube" if b.kind == "cube" else "pore"]
    for w, (axis, sign) in enumerate(FULL_DIRS):
        k0 = b.cell_at(corner[w])
        a1, a2 = [a for a in range(3) if a != axis]
        fw = _fin(64 * w, b.perm) // 64
        b.waves[("march_full", w)] = (fw, 64)
        for lane in range(64):
            k = k0.copy()
            k[a1] += 2 * (lane % 8)
            k[a2] += 2 * (lane // 8)
            b.marcher(_fin(64 * w + lane, b.perm), "march_full", b.at(k), 0, axis, sign)


def _march_lanes(b):
    """movers only in lane 0, only in lane 63, and in lanes 62 and 63 of otherwise resting waves.  The two of the last wave
    take their ranks in the pool from each other's ballot bit: each marches up to a rester of its own (0.5 cr ahead of it,
    on its line) in the last step in between of the second cycle — had both been given one node, one of the two pairs
    would not be found."""
    t_meet = 2 * b.K - 1
    for w, lanes in ((FULL_WAVES, (0,)), (FULL_WAVES + 1, (63,)), (FULL_WAVES + 2, (62, 63))):
        fw = _fin(64 * w, b.perm) // 64
        b.waves[("march_lanes", lanes)] = (fw, len(lanes))
        for lane in lanes:
            k = b.row()
            im = b.marcher(64 * fw + lane, "march_lanes", b.at(k), 0)
            if len(lanes) == 2:
                ir = _fin(b.mixed(1)[0], b.perm)
                b.rester(ir, "march_lanes_partner", b.at(k + np.array([t_meet, 0, 0]), (0.5 + 0.5 * b.u, 0.5, 0.5)), axis=0)
                b.meet.append((f"march_lanes_{lane}", im, ir, t_meet))


def _march_tail(b):
    b.waves[("march_tail", TAIL_MARCHERS)] = (WAVES, TAIL_MARCHERS)
    for q in range(N_MAIN + TAIL - TAIL_MARCHERS, N_MAIN + TAIL):
        b.marcher(q, "march_tail", b.at(b.row()), 0)


# Every pair below meets on ONE line, the marching axis: equal masses exchange their velocities along it, so after the hit
# the particles march on (or rest) on that line at a known fraction of a cell in the other two axes.
def _frac(axis, f):
    fr = [0.5, 0.5, 0.5]
    fr[axis] = f
    return fr


def _pair_pool_pool(b):
    """A marches up the axis, B down it: closer than cr for the first time after the streaming stages of the last step in
    between.  In one cell; across an x face; across a z face (cells of two z layers: the pair marches along z, on a line of
    its own 20 cells beside the rows)."""
    t, u = b.K - 1, b.u
    for name, axis, fa, fb in (("same", 0, 0.5 - 0.25 * u, 0.5 + 0.25 * u), ("x_adjacent", 0, 1.0 - 0.3 * u, 1.0 + 0.3 * u),
                               ("z_layers", 2, 1.0 - 0.3 * u, 1.0 + 0.3 * u)):
        k = b.row()
        if axis == 2:
            zmid = 0.5 * b.p.cube_z if b.kind == "cube" else 1.5 * b.p.dz
            k = np.array([k[0] - 20, k[1], b.cell_at([0.0, 0.0, zmid])[2]])
        ia, ib = b.mixed(2)
        ia, ib = _fin(ia, b.perm), _fin(ib, b.perm)
        b.marcher(ia, "pair_pool_pool", b.at(k, _frac(axis, fa)), t, axis, 1.0)
        b.marcher(ib, "pair_pool_pool", b.at(k, _frac(axis, fb)), t, axis, -1.0)
        b.meet.append(("pair_pool_pool_" + name, ia, ib, t))


def _pair_pool_rest(b):
    """M marches +x and arrives beside the rester R in the first step in between (its first pool node): R ahead of it in
    the same cell, behind it in the cell below, ahead of it in the cell above"""
    u = b.u
    for name, fm, fr in (("same", 0.5 - 0.25 * u, 0.5 + 0.25 * u), ("lower", 0.3 * u, -0.3 * u), ("higher", 1.0 - 0.3 * u, 1.0 + 0.3 * u)):
        for m_first in (True, False):
            k = b.row()
            lo, hi = b.ordered(2)
            im, ir = (lo, hi) if m_first else (hi, lo)
            b.marcher(im, "pair_pool_rest", b.at(k, _frac(0, fm)), 1, 0, 1.0)
            b.rester(ir, "pair_pool_rest", b.at(k, _frac(0, fr)), axis=0)
            b.meet.append((f"pair_pool_rest_{name}_{'below' if m_first else 'above'}", im, ir, 1))


def _turned_round(b, case, k, axis, meet_at):
    """P leaves cell A = k in step 1 along +axis, meets Q head-on in B (0.5 cr apart: both end 0.5 cr further out with
    their velocities swapped), and is back in A in step 2, 0.5 cr short of where it was in step 0.  meet_at 2: the rester R
    waits on the line 0.7 cr beyond that point — 1.2 cr from P in step 0, in range from step 2 on, when A's list holds P's
    dead node and its live one; 3: R waits one cell further back, 0.5 cr beyond where P arrives in step 3."""
    e = np.eye(3)[axis]
    cr, h = b.cr, b.h
    p1 = b.at(k, _frac(axis, 0.7)) + h * e            # P after the streaming stages of step 1: in B
    ip, iq, ir = [_fin(r, b.perm) for r in b.mixed(3)]
    b.marcher(ip, case, p1, 1, axis, 1.0)
    b.marcher(iq, case, p1 + 0.5 * cr * e, 1, axis, -1.0)
    back = p1 - 0.5 * cr * e - h * e                  # P after the streaming stages of step 2: in A again
    b.rester(ir, case, back - 0.7 * cr * e if meet_at == 2 else back - h * e - 0.5 * cr * e, axis=axis)
    b.meet.append((case + "_turn", ip, iq, 1))
    b.meet.append((case, ip, ir, meet_at))
    a = b.cell_at(b.at(k))
    b.cells_of.append((case, ip, [a, a + e.astype(np.int64), a]))


def _there_and_back(b):
    if b.kind != "cube":
        _turned_round(b, "there_and_back", b.row(), 0, 2)
        return
    # off the wall x = 0 (cell 1 is [0, h)), 1.5 h per step: at 1.63 h, at 0.13 h, then 1.37 h beyond the wall, reflected.
    # R rests on the line 0.7 cr nearer the wall than that: 1.2 cr or more from P in step 0, in cell 2 as well
    k = b.row()
    cr, h = b.cr, b.h
    yz = b.at(k)
    ip, ir = [_fin(r, b.perm) for r in b.mixed(2)]
    d = np.array([-1.5 * h, 0.0, 0.0])
    b.put(ip, "there_and_back", np.array([1.63 * h, yz[1], yz[2]]) - d, d / b.dt)
    b.rester(ir, "there_and_back", [1.37 * h - 0.7 * cr, yz[1], yz[2]], axis=0)
    b.meet.append(("there_and_back", ip, ir, 2))
    a = np.array([2, k[1], k[2]])
    b.cells_of.append(("there_and_back", ip, [a, a - np.array([1, 0, 0]), a]))


def _rebound_mover(b):
    _turned_round(b, "rebound_mover", b.row(), 0, 3)


def _layer_window(b):
    """pore: across the first narrow layer's lower face, inside the pore mouth (r < R_p_c): U upwards to a rester in the body
    layer, D downwards to a rester in the cap layer (each 0.5 cr ahead of it on its line), and P there and back"""
    G, h, u = b.G, b.h, b.u
    kb = int(np.flatnonzero(G.lay_n < G.gx)[0])        # the first body layer; kb - 1 keeps the full window
    d = 0.5 * b.p.dx
    for name, (x, y), sign in (("up", (d - 3 * h, d - 3 * h), 1.0), ("down", (d + 3 * h, d - 3 * h), -1.0)):
        k = b.cell_at([x, y, 0.0])
        k[2] = kb if sign > 0 else kb - 1               # where it is after the streaming stages of step 1
        im, ir = b.ordered(2)
        b.marcher(im, "layer_window", b.at(k, _frac(2, 0.5 - sign * 0.25 * u)), 1, 2, sign)
        b.rester(ir, "layer_window", b.at(k, _frac(2, 0.5 + sign * 0.25 * u)), axis=2)
        b.meet.append(("layer_window_" + name, im, ir, 1))
        b.cells_of.append(("layer_window_" + name, im, [k - np.array([0, 0, int(sign)]), k]))
    k = b.cell_at([d - 3 * h, d + 3 * h, 0.0])
    k[2] = kb - 1
    _turned_round(b, "layer_window_back", k, 2, 2)


def _bounds_jump(b):
    """pore: a particle between R_oa_c and R_oa flying along a tangent — the wall's contact solve has no root, it is left
    alone — is beyond R_oa after the drift of step 1 and put on the axis by the bounds check; R waits 0.5 cr ahead of it"""
    p, h = b.p, b.h
    z = b.at(b.cell_at([0.0, 0.0, 0.5 * p.dz]))[2]
    y0 = np.sqrt(p.R_oa_sq - 2.5 * h * h)               # after step 0: R_oa^2 - 1.5 h^2, after step 1: R_oa^2 + 1.5 h^2
    ip, ir = [_fin(r, b.perm) for r in b.mixed(2)]
    d = np.array([h, 0.0, 0.0])
    b.put(ip, "bounds_jump", [0.0, y0, z], d / b.dt)
    b.rester(ir, "bounds_jump", [0.5 * b.cr, 0.0, z], axis=0)
    b.meet.append(("bounds_jump", ip, ir, 1))


def catalogue(kind, perm, cell, K, shift=0, pad=0):
    """every case in one state of 805 particles (plus shift + pad resters), for a cycle of K steps.  kind "temp", the
    energised pore: the marching waves, the pool-pool pairs and the layer window, all in open space, far from every
    energised surface (no case 3 .. 9 ever fires)."""
    b = _Builder(kind, perm, cell, K)
    _march_full(b); _march_lanes(b); _march_tail(b)
    _pair_pool_pool(b)
    if kind != "temp":
        _pair_pool_rest(b); _there_and_back(b); _rebound_mover(b)
    if kind != "cube":
        _layer_window(b)
    if kind == "pore":
        _bounds_jump(b)
    return b.finish("limits", shift, pad)


def face_rounding(kind, cell):
    """A state of its own (one resting wave): a particle that creeps across a grid face so that after step 1 its double
    position is below the face while its single-precision record is on it, and a partner 0.5 cr across the face in that
    step.  The partner marches past along y instead of resting there: a rester 0.5 cr beyond the face would be within range
    of the creeping particle (0.01 h per step) from step 0 on, and their hit would end the creep before it reaches the
    face.  Only the physics is asserted on it."""
    b = _Builder(kind, "identity", cell, 4)
    G, h, dt = b.G, b.h, b.dt
    k = b.row()
    creep = 0.01 * h
    found = None
    for dk in range(40):
        face_rel = (k[0] + dk) * h
        for below in around(G.x0 + face_rel, 6)[:6]:
            rel = below - G.x0
            if np.floor(rel * G.inv_h) == k[0] + dk - 1 and \
                    np.floor((G.x0 + np.float64(np.float32(rel)) - G.x0) * G.inv_h) == k[0] + dk:
                # a start from which two drifts of the same velocity land exactly there
                v = creep / dt
                for start in around(below - 2.0 * (dt * v), 16):
                    if (start + dt * v) + dt * v == below:
                        found = (dk, below, start, v)
                        break
            if found:
                break
        if found:
            break
    assert found, "no face whose single-precision neighbourhood rounds up"
    dk, below, start, v = found
    yz = b.at(k)
    ip, ir = 5, 70 % 64 + 20
    b.put(ip, "face_rounding", [start, yz[1], yz[2]], [v, 0.0, 0.0])
    # (the partner across the face passes by along y: a cell away before step 1, so the creeping particle is undisturbed)
    b.marcher(ir, "face_rounding", [below + 0.5 * b.cr, yz[1], yz[2]], 1, 1, 1.0)
    b.meet.append(("face_rounding", ip, ir, 1))
    n_keep = 64
    # (one wave: the builder's layout is cut down to it)
    spots = iter(b._filler_spots())
    s = EdgeState(b.p, dt)
    for q in range(n_keep):
        if q not in b.spec:
            b.rester(q, "filler", next(spots))
        case, st, vel = b.spec[q]
        s.add(case, *st, *vel, flag=1, landed=False, jitter=False)
    s.finish()
    s.p.fine_cell, s.p.detect_mode, s.p.reserved1 = b.h_asked, 1, 1
    s.extra.update(kind=kind, perm="identity", K=4, h=h, h_asked=b.h_asked, which="face_rounding", meet=list(b.meet),
                   cells_of=[], waves={}, on_face=(ip, float(below), int(k[0] + dk)))
    return s


# ---------------------------------------------------------------------------------------------------------------- the oracle's run
COUNTERS = ("n_pp", "n_wall", "n_oob_walls", "n_oob_pp", "n_paths", "n_fp_errors")


class Tape:
    """The oracle taken through a state step by step: ``whole`` by timestep(), ``staged`` through the step's stages one by
    one, for the positions after the streaming stages and before the sweep; the two must agree after every step."""

    def __init__(self, O, s):
        self.s, self.pore = s, s.p.geometry != 1
        self.whole, self.staged = O.Oracle(s.p, mode="mul"), O.Oracle(s.p, mode="mul")
        a = s.arrays()
        self.set_state(dict(zip(STATE + ["flag"], a)))

    def set_state(self, st):
        for o in (self.whole, self.staged):
            o.upload(*[st[k] for k in STATE], flag=st["flag"])

    def state(self):
        return self.whole.state()

    def step(self):
        """dict(pre = (x, y, z) after the streaming stages, state = after the step, stats, rec = the step's records)"""
        s, whole, staged = self.s, self.whole, self.staged
        rc, st = whole.timestep(s.dt)
        assert rc == 0, rc
        staged.drift(s.dt)
        if self.pore:
            rc2, _ = staged.pore_walls()
            assert rc2 == 0
            staged.bounds(False)
        else:
            staged.cube_walls()
        pre = tuple(staged.arr[k].copy() for k in ("x", "y", "z"))
        assert staged.sweep()[0] == 0
        if self.pore:
            staged.bounds(False)
        staged.step += 1
        staged.drain_paths()
        state = whole.state()
        for k in STATE:
            assert np.array_equal(state[k], staged.arr[k]), k
        return dict(pre=pre, state=state, stats={k: st[k] for k in COUNTERS}, rec=whole.drain_paths())


class TempTape:
    """The energised pore's step (Temp:662-853) through the oracle's stages, for states in which no energised case fires:
    nothing random is left in such a step."""

    def __init__(self, O, s):
        self.s = s
        self.o = O.Oracle(s.p, mode="mul")
        a = s.arrays()
        self.o.upload(*a[:10], flag=a[10])

    def step(self):
        o, dt = self.o, self.s.dt
        o.drift(dt, True)
        errs = o.temp_specular()
        for case in range(3, 10):
            assert len(o.wall_hits(case)[0]) == 0, case
        oob1 = o.bounds(True)
        pre = tuple(o.arr[k].copy() for k in ("x", "y", "z"))
        rc, npp, _ = o.sweep()
        assert rc == 0
        oob2 = o.bounds(True)
        o.step += 1
        rec = o.drain_paths()
        return dict(pre=pre, state=o.state(), rec=rec,
                    stats=dict(n_pp=npp, n_wall=0, n_oob_walls=oob1, n_oob_pp=oob2, n_paths=len(rec), n_fp_errors=errs))


def oracle_run(O, s, nsteps):
    """the state through the oracle: one dict per step (Tape.step)"""
    tape = TempTape(O, s) if s.extra["kind"] == "temp" else Tape(O, s)
    return [tape.step() for _ in range(nsteps)]


def close_pairs(s, pre):
    """the pairs i < j closer than one collision range at the positions pre, and the distances inside the forbidden band"""
    P = np.stack(pre, axis=1)
    d = P[:, None, :] - P[None, :, :]
    D = np.sqrt((d * d).sum(axis=2))
    cr = s.p.collision_range
    i, j = np.nonzero(np.triu(D < cr, k=1))
    band = np.triu((D >= 0.9 * cr) & (D <= 1.1 * cr), k=1)
    return np.stack([i, j], axis=1), D[band] / cr


def face_margin(s, pre, among=None):
    """the smallest distance of a particle (of those in the mask `among`) from a grid face, in cells"""
    G = grid_of(s.p, s.extra["h_asked"])
    m = 1.0
    for v, o in zip(pre, (G.x0, G.y0, G.z0)):
        f = (v - o) * G.inv_h
        f = np.minimum(f - np.floor(f), 1.0 - (f - np.floor(f)))
        m = min(m, float(f.min() if among is None else f[among].min()))
    return m


def hit_pairs(rec):
    pp = rec[rec["j"] >= 0]
    return {(int(min(i, j)), int(max(i, j))) for i, j in zip(pp["i"], pp["j"])}


def catalogue_proofs(s, run):
    """On the CPU: the distance rule and the face margin hold in every step; the mirror's counters of the marching waves
    are the intended ones; every named pair meets in the oracle's records in its step, not before; the particles that leave
    and come back are filed under the cells meant.  Returns (counts[t, wave], candidates per step)."""
    K, h = s.extra["K"], s.extra["h_asked"]
    pre = [r["pre"] for r in run]
    assert len(pre) == steps(K)
    ncand = []
    for t, q in enumerate(pre):
        pairs, band = close_pairs(s, q)
        assert band.size == 0, (t, band)
        if s.extra["which"] != "face_rounding":
            assert face_margin(s, q) >= 1.0e-3, (t, face_margin(s, q))
        ncand.append(len(pairs))
    counts, outside = movers_per_wave(s.p, h, pre, K)
    assert not outside.any()
    for (case, _), (wave, per_step) in s.extra["waves"].items():
        for t in range(len(pre)):
            assert counts[t, wave] == per_step * (t % K), (case, wave, t, counts[t, wave])
    for case, i, j, t in s.extra["meet"]:
        key = (min(i, j), max(i, j))
        first = [q for q in range(len(run)) if key in hit_pairs(run[q]["rec"])]
        if case == "bounds_jump":
            assert first and first[0] in (t, t + 1), (case, first)
        else:
            assert first and first[0] == t, (case, i, j, t, first)
    G = grid_of(s.p, h)
    for case, i, cells in s.extra["cells_of"]:
        want = [int(grid_cell(G, *np.array(c)[:, None])[0][0]) for c in cells]
        got = [int(grid_cell(G, *grid_coords(G, *[v[i:i + 1] for v in pre[t]]))[0][0]) for t in range(len(cells))]
        assert got == want, (case, i, got, want)
    return counts, ncand
