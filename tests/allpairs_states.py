"""Crafted states for the two all-pairs detectors in front of the grid resolve (detect_mode = 2, amc_grid.hip):
k_detect_allpairs (tiles of AP_T = 256 particles, direct d^2) and k_detect_allpairs_tiled (tiles of AP2_T = 1024, AP2_R = 4
particles i per thread in registers, j walked in chunks of AP2_CHUNK = 8, the expanded form |ri|^2 + |rj|^2 - 2 ri.rj against
a raised threshold).

Pure NumPy and deterministic, in the style of tests/edge_states.py.  New here: the builder decides WHICH PARTICLE INDEX every
crafted particle gets — what the kernels' tile pair, register row, chunk and diagonal rule are functions of.  Every other
index is a *filler*: a slow particle on a lattice of more than eight collision ranges (cr), with every lattice site within
five cr of a crafted particle left empty.  Crafted particles move by less than 0.1 cr in the four steps a test runs.

A crafted pair is two particles at one of the separations of ``edge_states._separations`` (in_1, in_2, in_3, in_8: inside the
collision range by m * 2^-52 relative; on; above_1; above_far).  Coordinates of 1e-8 .. 3e-6 m cannot carry a separation to
2^-52 of cr, so after the first try one coordinate of one partner is moved ulp by ulp until the overlap test of Pore:173-174
(``distance_lt``) says what the name says: in_* overlap by as little as the coordinates allow, on / above_* do not.  (The
pairs of ``outside`` are left as ``edge_states.outside_pairs`` makes them.)

Where a tile has fewer particles than pairs to carry (a last tile of 5, of 1), or where the point is one particle with several
hits (the chunk re-walk in ``switch_sizes``), a particle has up to three partners: a *star*.
Its centre rests, its leaves lie along +x, +y and +z and approach along their own axis only, so a collision with one leaf
moves the centre along that leaf's axis alone, by the pair's gap cr - d, and the squared distance to the other leaves by the
square of that — not at all in doubles.  What ``collide`` says of each pair of a star therefore holds whichever pair the sweep takes first.

``extra`` of every state: ``pairs`` (i, j) with i > j, ``collide`` (distance_lt at the positions the sweep sees), ``names``
(separation name per pair), ``tiles`` (bi, bj) per pair, ``offsets`` (i, j in their tiles), ``T`` (the tile of the kernel
that runs at this n), ``filler`` (mask), ``diag`` (the diagonal classes per pair, '' elsewhere)."""
from __future__ import annotations

from fractions import Fraction

import numpy as np

from argon_monte_carlo_amd import params as PR
from tests.edge_states import EdgeState, _separations, distance_lt, land
from tests.list_states import grid_of

# the kernels' constants (tests/test_allpairs_states_host.py reads them from amc_grid.hip and compares)
AP_T = 256
AP2_T = 1024
AP2_R = 4
AP2_THREADS = AP2_T // AP2_R
AP2_CHUNK = 8
SWITCH_N = 16 * AP2_T             # amc_launch_detect: the tiled kernel from this n on (with a grid)
CR2_INFLATE = 1.0 + 1.0e-9        # AMC_CR2_INFLATE: both kernels' cr^2 before the tiled kernel raises it further

IN = ("in_1", "in_2", "in_3", "in_8")
OUT = ("on", "above_1", "above_far")
FINE_MULT = 2.01 * 1.02           # fine_cell in collision ranges: the smallest the library takes
DIRS = dict(face=(1.0, 0.0, 0.0), edge=(1.0, 1.0, 0.0), corner=(1.0, 1.0, 1.0))
MATRIX = [("cube", AP2_T, 17, 544), ("pore", AP2_T, 17, 544), ("cube", AP_T, 7, 5)]


def tile_of(n):
    """the tile of the kernel amc_launch_detect picks for n particles (cube and pore: there is a grid)"""
    return AP2_T if n >= SWITCH_N else AP_T


def boundary_offsets(T, size):
    """the in-tile offsets the kernels' own structure makes special, for a tile holding `size` of its T particles: 0 and
    T - 1, the chunk boundary 7 | 8, the register-row boundaries 255 | 256, 511 | 512, 767 | 768, the last valid index"""
    b = [0, T - 1, AP2_CHUNK - 1, AP2_CHUNK]
    if T == AP2_T:
        for r in range(1, AP2_R):
            b += [r * AP2_THREADS - 1, r * AP2_THREADS]
    b.append(size - 1)
    return sorted({o for o in b if o < size})


def _params(kind):
    p, c = PR.pore_params(n=0) if kind == "pore" else PR.cube_params(n=0, cube_side=100.0e-9, n_sub=15)
    p.fine_cell = FINE_MULT * p.collision_range
    p.detect_mode = 2
    return p, c


def _sites(kind, p, need):
    """lattice sites, more than 8 cr apart: the cube's whole volume; in the pore a square column inside R_p over the whole
    height, so that crafted pairs stand at every distance from the detection grid's origin"""
    if kind == "cube":
        g = np.linspace(5.0e-9, p.cube_x - 5.0e-9, 26)
        X, Y, Z = np.meshgrid(g, g, g, indexing="ij")
    else:
        gxy = np.arange(-5, 6) * 3.4e-9 + 0.7e-9
        gz = np.linspace(6.0e-9, p.H - 6.0e-9, int(np.ceil(need / len(gxy) ** 2)) + 1)
        Z, X, Y = np.meshgrid(gz, gxy, gxy, indexing="ij")
    s = np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1)
    assert len(s) >= need, (len(s), need)
    return s


def _land3(pos, vel, dt):
    out = [land(t, v, dt) for t, v in zip(pos, vel)]
    return None if any(c is None for c in out) else [float(c) for c in out]


def exact_margin(a, b, cr):
    """cr^2 - d^2 of two positions, exactly (as a float at the end)"""
    d2 = sum((Fraction(float(q)) - Fraction(float(r))) ** 2 for q, r in zip(a, b))
    return float(Fraction(float(cr)) ** 2 - d2)


class _Build:
    """crafted rows by particle index, then fillers on what is left of the lattice"""

    def __init__(self, kind, n, landed=True):
        self.kind, self.n, self.landed = kind, int(n), landed
        self.p, c = _params(kind)
        self.dt = c["dt"]
        self.cr = self.p.collision_range
        self.vrel = 0.02 * self.cr / self.dt           # 0.01 cr per particle and step
        self.rows, self.at = {}, {}                    # index -> (case, start, velocity); index -> position at the sweep
        self.pairs, self.want, self.names = [], [], []
        self.T = tile_of(self.n)

    # ---- geometry
    def _put(self, idx, case, start, vel, at):
        assert 0 <= idx < self.n and idx not in self.rows, (case, idx)
        self.rows[idx] = (case, [float(v) for v in start], [float(v) for v in vel])
        self.at[idx] = [float(v) for v in at]

    def _settle(self, a, b, va, vb, want, axis):
        """move b[axis] ulp by ulp, towards a or away from it, until the overlap test says `want` and both particles land:
        returns the two start positions and the two positions at the sweep"""
        a, b = [float(v) for v in a], [float(v) for v in b]
        toward = -np.inf if b[axis] > a[axis] else np.inf
        for _ in range(64):
            if bool(distance_lt(*a, *b, self.cr)) == want:
                sa, sb = _land3(a, va, self.dt), _land3(b, vb, self.dt)
                if sa is not None and sb is not None:
                    return sa, sb, a, b
            b[axis] = float(np.nextafter(b[axis], toward if want else -toward))
        raise AssertionError(("cannot settle", a, b, want))

    def _record(self, i, j, name, want):
        assert i > j, (i, j)
        self.pairs.append((i, j))
        self.names.append(name)
        self.want.append(want)

    def pair(self, i, j, ctr, dname, sname, case):
        """two particles straddling ctr along DIRS[dname] as edge_states.grid_pairs places them, but approaching, slowly: the
        contact time Pore:185 takes (the larger root) is then the one just past, cr - d over the closing speed, and the
        collision moves neither particle by more than that gap"""
        sep = dict(_separations(self.cr))[sname]
        u = np.array(DIRS[dname]) / np.linalg.norm(DIRS[dname])
        a = np.asarray(ctr, dtype=np.float64) - 0.5 * sep * u
        b = a + sep * u
        drift = np.array([1.0e-3 * (len(self.pairs) % 97), 0.05, 0.02]) * self.vrel        # (no two pairs share a velocity)
        va, vb = 0.5 * self.vrel * u + drift, -0.5 * self.vrel * u + drift
        want = sname in IN
        # (the coordinate with the coarsest ulp is the one that can carry the pair across the threshold)
        axis = max((k for k in range(3) if u[k] != 0.0), key=lambda k: abs(b[k]))
        sa, sb, a, b = self._settle(a, b, va, vb, want, axis)
        self._put(j, case, sa, va, a)
        self._put(i, case, sb, vb, b)
        self._record(i, j, sname, want)

    def star(self, centre, leaves, ctr, case):
        """a resting centre with up to three leaves (index, separation name) on +x, +y, +z, each approaching along its axis"""
        assert 2 <= len(leaves) <= 3
        ctr = [float(v) for v in ctr]
        zero = [0.0, 0.0, 0.0]
        self._put(centre, case, ctr, zero, ctr)
        for axis, (j, sname) in enumerate(leaves):
            sep = dict(_separations(self.cr))[sname]
            b = list(ctr)
            b[axis] = ctr[axis] + sep
            vb = list(zero)
            vb[axis] = -self.vrel * (1.0 + 1.0e-3 * (len(self.pairs) % 97))
            want = sname in IN
            _, sb, _, b = self._settle(ctr, b, zero, vb, want, axis)
            self._put(j, case, sb, vb, b)
            self._record(max(centre, j), min(centre, j), sname, want)

    def realise(self, specs, case="pair"):
        """specs (i, j, separation name) with i > j: single pairs (directions face, edge, corner in turn) and stars, each on
        a lattice site of its own, spread evenly through the lattice"""
        deg = {}
        for i, j, _ in specs:
            assert i > j
            deg[i] = deg.get(i, 0) + 1
            deg[j] = deg.get(j, 0) + 1
        groups, centre_of = [], {}
        for i, j, sname in specs:
            c = i if deg[i] > 1 else (j if deg[j] > 1 else None)
            if c is None:
                groups.append(("pair", i, j, sname))
                continue
            assert deg[j if c == i else i] == 1, ("not a star", i, j)
            if c not in centre_of:
                centre_of[c] = len(groups)
                groups.append(("star", c, []))
            groups[centre_of[c]][2].append((j if c == i else i, sname))
        sites = _sites(self.kind, self.p, self.n + len(groups) + 64)
        stride = len(sites) // len(groups)
        for g, grp in enumerate(groups):
            ctr = sites[g * stride + stride // 2]
            if grp[0] == "pair":
                self.pair(grp[1], grp[2], ctr, ("face", "edge", "corner")[g % 3], grp[3], case)
            else:
                self.star(grp[1], grp[2], ctr, case + "_star")

    # ---- the state
    def finish(self, extra=None):
        cr, n = self.cr, self.n
        crafted = np.array(sorted(self.rows), dtype=np.int64)
        C = np.array([self.at[i] for i in crafted])
        sites = _sites(self.kind, self.p, n + 64)
        free = np.ones(len(sites), dtype=bool)
        for q in C:                                     # every site within 5 cr of a crafted particle stays empty
            free &= ((sites - q) ** 2).sum(axis=1) >= (5.0 * cr) ** 2
        sites = sites[free]
        nfill = n - len(crafted)
        assert len(sites) >= nfill, (len(sites), nfill)
        pick = sites[(np.arange(nfill) * len(sites)) // max(nfill, 1)]          # spread over the whole lattice
        s = EdgeState(self.p, self.dt)
        filler = np.ones(n, dtype=bool)
        filler[crafted] = False
        f = 0
        for i in range(n):
            if filler[i]:
                v = [0.3 * (1 + i % 3), -0.2 * (1 + i % 2), 0.1 * (1 + i % 5)]  # (below 1 m/s: 1e-3 cr per step in the pore, 0.02 in the cube)
                got = s.add("filler", *pick[f], *v, landed=False, jitter=False)
                f += 1
            else:
                case, start, vel = self.rows[i]
                got = s.add(case, *start, *vel, landed=False, jitter=False)
            assert got == i
        st = s.finish()
        X = [st.x + self.dt * st.vx, st.y + self.dt * st.vy, st.z + self.dt * st.vz] if self.landed else [st.x, st.y, st.z]
        P = np.array(self.pairs, dtype=np.int64).reshape(-1, 2)
        for k in range(3):                              # the crafted particles are where they were settled, bit for bit
            assert np.array_equal(X[k][crafted], C[:, k])
        col = np.asarray(distance_lt(X[0][P[:, 0]], X[1][P[:, 0]], X[2][P[:, 0]], X[0][P[:, 1]], X[1][P[:, 1]], X[2][P[:, 1]], cr))
        for k, w in enumerate(self.want):
            assert w is None or bool(col[k]) == w, (k, self.pairs[k], self.names[k])
        # fillers keep clear of every crafted particle (4 cr), crafted particles of every other pair (3 cr)
        A = np.stack(X, axis=1)
        mate = {}
        for i, j in self.pairs:
            mate.setdefault(i, set()).add(j)
            mate.setdefault(j, set()).add(i)
        for i in crafted:
            d2 = ((A - A[i]) ** 2).sum(axis=1)
            near = np.flatnonzero(d2 < (4.0 * cr) ** 2)
            own = {int(i)} | mate[int(i)] | set().union(*[mate[m] for m in mate[int(i)]])
            assert not filler[near].any(), (int(i), near)
            assert all(int(q) in own or d2[q] >= (3.0 * cr) ** 2 for q in near), (int(i), near)
        T = self.T
        st.extra.update(pairs=P, collide=col, names=list(self.names), tiles=P // T, offsets=P % T, T=T, filler=filler,
                        diag=[""] * len(P), kind=self.kind)
        st.extra.update(extra or {})
        return st


# ---------------------------------------------------------------------------------------------------------- tile matrix
class _Pool:
    """free in-tile offsets of one tile: the kernels' boundaries first (register rows first for a particle in the i role,
    chunks first in the j role), then every other chunk boundary 8k - 1 | 8k; role d (a diagonal tile's own pair, which has
    its classes besides) the other way round, so that the boundaries go to the off-diagonal pairs"""

    def __init__(self, T, size, t=0):
        self.T, self.size, self.used = T, size, set()
        rows = [o for r in range(1, AP2_R) for o in (r * AP2_THREADS - 1, r * AP2_THREADS)] if T == AP2_T else []
        ends = [size - 1, 0] if size < T else [0, T - 1]
        chunk = [AP2_CHUNK - 1, AP2_CHUNK]
        rest = [o for k in range(2, T // AP2_CHUNK + 1) for o in (AP2_CHUNK * k - 1, AP2_CHUNK * k)]
        if size < 4 * AP2_CHUNK:
            rest = list(range(size))
        mine = [ends[(t // 2) % 2]]            # (the i role takes one end of the tile and leaves the other to the j role)
        self.order = dict(i=rows + mine + rest + chunk + ends, j=chunk + ends + rows + rest, d=rest + chunk + ends + rows)

    def take(self, role, exact=None):
        for o in ([exact] if exact is not None else self.order[role]):
            if 0 <= o < self.size and o not in self.used:
                self.used.add(o)
                return o
        return None


def tile_matrix(kind, T, ntiles, last):
    """n = (ntiles - 1) T + last.  One colliding pair (in_1, in_2, in_3, in_8 in turn) with i in tile bi and j in tile bj
    for EVERY tile pair bj <= bi; on every third tile pair that still has two free particles a second pair at on, above_1 or
    above_far; the in-tile offsets taken from the kernels' boundaries first (_Pool).  Every diagonal tile also gets, where
    its size allows, i = j + 1 across a chunk boundary ('adjacent'), i = j + 256 k — one thread, register rows 0 and k —
    ('same_thread', T = 1024 only) and, on even tiles, i = last particle of the tile, j = 0 ('ends'; an index has one pair,
    so the odd tiles leave 0 and T - 1 to the off-diagonal pairs).  A tile too small for its pairs shares particles (stars)."""
    n = (ntiles - 1) * T + last
    assert tile_of(n) == T and 0 < last <= T
    b = _Build(kind, n)
    size = [T] * (ntiles - 1) + [last]
    pool = [_Pool(T, s, t) for t, s in enumerate(size)]
    specs, diag, i_role = [], {}, {t: [] for t in range(ntiles)}
    deg = {}

    def spec(i, j, sname, cls=""):
        specs.append((i, j, sname))
        diag[(i, j)] = cls
        deg[i] = deg.get(i, 0) + 1
        deg[j] = deg.get(j, 0) + 1

    q = 0
    for bi in range(ntiles):
        # diagonal classes first: they need particular offsets
        ends = False
        if size[bi] >= 2 * AP2_CHUNK + 2:
            k = 2 + bi % 5
            oj, oi = pool[bi].take("j", AP2_CHUNK * k - 1), pool[bi].take("i", AP2_CHUNK * k)
            spec(bi * T + oi, bi * T + oj, IN[bi % 4], "adjacent")
        if T == AP2_T:
            k = 1 + bi % (AP2_R - 1)
            while k > 1 and 100 + bi + k * AP2_THREADS >= size[bi]:
                k -= 1
            if 100 + bi + k * AP2_THREADS < size[bi]:
                oj = pool[bi].take("j", 100 + bi)
                oi = pool[bi].take("i", 100 + bi + k * AP2_THREADS)
                spec(bi * T + oi, bi * T + oj, IN[(bi + 1) % 4], "same_thread")
        if bi % 2 == 0 and size[bi] >= 2:
            oj, oi = pool[bi].take("j", 0), pool[bi].take("i", size[bi] - 1)
            spec(bi * T + oi, bi * T + oj, IN[(bi + 2) % 4], "ends")
            i_role[bi].append(bi * T + oi)
            ends = True
        # (the boundaries go to the off-diagonal pairs first; a small tile keeps two particles for its diagonal pair first)
        for bj in ([bi] + list(range(bi)) if size[bi] < ntiles + 4 else range(bi + 1)):
            if bi == bj and ends and size[bi] < AP2_CHUNK:
                continue                                  # (a tile of a few particles: its one diagonal pair is the 'ends' pair)
            # (nothing is above the last tile: the j role of its own pair is the only one its chunk boundary 7 | 8 can have)
            role = "j" if bi == ntiles - 1 else "d"
            oj = pool[bj].take(role if bi == bj else "j")
            oi = pool[bi].take(role if bi == bj else "i")
            if oj is None and bi == bj:
                raise AssertionError(("no free pair in tile", bi))
            if oi is None:                                # the tile is used up: a particle already in the i role takes another partner
                i = min((c for c in i_role[bi] if deg[c] < 3), key=lambda c: (deg[c], -c))
            else:
                i = bi * T + oi
                i_role[bi].append(i)
            j = bj * T + oj
            if i < j:
                i, j = j, i
            spec(i, j, IN[q % 4])
            q += 1
    nprimary = len(specs)
    # pairs that must not collide
    second = 0
    q = 0
    for bi in range(ntiles):
        for bj in range(bi + 1):
            q += 1
            if q % 3:
                continue
            free_i = pool[bi].size - len(pool[bi].used)
            free_j = pool[bj].size - len(pool[bj].used)
            if (bi == bj and free_i < 2) or free_i < 1 or free_j < 1:
                continue
            oj, oi = pool[bj].take("j"), pool[bi].take("i")
            i, j = bi * T + oi, bj * T + oj
            spec(max(i, j), min(i, j), OUT[second % 3])
            second += 1
    assert 4 * second >= ntiles * (ntiles + 1) // 2, second
    b.realise(specs)
    st = b.finish()
    st.extra["diag"] = [diag[(int(i), int(j))] for i, j in st.extra["pairs"]]
    st.extra["ntiles"] = ntiles
    assert nprimary >= ntiles * (ntiles + 1) // 2
    return st


def tile_pairs_covered(s):
    """the tile pairs (bi, bj) on which a crafted pair collides"""
    return {(int(a), int(c)) for (a, c), hit in zip(s.extra["tiles"], s.extra["collide"]) if hit}


# ---------------------------------------------------------------------------------------------------------- the switch
def switch_sizes():
    """three cube states around the switch between the two kernels: n = 16383 (the 256 kernel's largest launch: 64 tiles,
    the last with 255 particles), 16384 (sixteen full 1024 tiles, no padding), 16385 (a 17th tile of one particle).  Sixteen
    colliding pairs and four that must not collide, among them (n - 1, 0) and (n - 1, n - 2) — a star round n - 1 —, a pair
    inside the last full tile, pairs across the boundaries of both kernels' tiles, and two stars for the chunk re-walk of the
    tiled kernel (extra["rewalk"]): ``same_chunk`` — one i whose three partners j stand in one chunk of 8, so the re-walk has
    to push more than the pair that raised the flag — and ``same_thread`` — one j whose three partners i = i0 + 256 r are
    the register rows 1, 2, 3 of one thread, so one j read has to push three pairs."""
    out = []
    for n in (SWITCH_N - 1, SWITCH_N, SWITCH_N + 1):
        b = _Build("cube", n)
        T = b.T
        F = ((n // T) - 1) * T                          # first index of the last full tile (16383: tile 62; 16384, 16385: tile 15)
        specs = [(n - 1, 0, "in_1"), (n - 1, n - 2, "in_2"), (F + T - 3, F + 1, "in_3"), (F + AP2_CHUNK, F + AP2_CHUNK - 1, "in_8"),
                 (9100, 1, "in_1"), (AP2_T, AP2_T - 1, "in_2"), (AP_T, AP_T - 1, "in_3"), (8200, 4100, "in_8"),
                 (14 * AP2_T, 14 * AP2_T - 1, "in_1"), (51 * AP_T, 51 * AP_T - 1, "in_2"),
                 (9500, 2, "on"), (12000, 11999, "above_1"), (n - 5, 3, "on"), (F + (300 % T), F + 40, "above_far")]
        rewalk = dict(same_chunk=(13000, [5 * AP2_CHUNK, 5 * AP2_CHUNK + 1, 5 * AP2_CHUNK + 2]),
                      same_thread=(5, [8 * AP2_T + 40 + r * AP2_THREADS for r in (1, 2, 3)]))
        for centre, leaves in rewalk.values():
            specs += [(max(centre, q), min(centre, q), IN[k]) for k, q in enumerate(leaves)]
        b.realise(specs)
        out.append(b.finish(dict(last_full_tile=F // T, rewalk=rewalk)))
    return out


# ---------------------------------------------------------------------------------------------------------- the far corner
def _spread_indices(q, T, n):
    """indices for crafted pair q, in tiles that change from pair to pair"""
    ntiles = (n + T - 1) // T
    bi, bj = (ntiles - 1) - q % 9, (5 * q) % ntiles
    i, j = bi * T + 10 + 3 * q, bj * T + 201 + 3 * q
    assert max(i, j) < n
    return max(i, j), min(i, j)


def far_corner(kind, n=16 * AP2_T + 544):
    """The face / edge / corner x _separations pairs of edge_states.grid_pairs at the point of the domain farthest from the
    detection grid's origin (the pore: 0.6 R_oa in x and y, 20 cells below z = H; the cube: its far corner) — where the
    expanded form |ri|^2 + |rj|^2 - 2 ri.rj cancels most — and the same set next to the origin.  extra["band"] = 2^-53
    (ex^2 + ey^2 + ez^2) of the grid's extent, the scale of one rounding of the expanded form; extra["margin"] = cr^2 - d^2
    per pair (exact); extra["anchor"] = 'far' or 'origin' per pair; extra["thr"] = the kernel's raised threshold."""
    assert n >= SWITCH_N
    b = _Build(kind, n)
    p, cr = b.p, b.cr
    G = grid_of(p, p.fine_cell)
    h = G.h
    xlo, xhi, zhi = (-p.R_oa, p.R_oa, p.H) if kind == "pore" else (0.0, p.cube_x, p.cube_z)

    def face(o, v):                      # the grid face at or below v
        return o + np.floor((v - o) / h) * h

    if kind == "pore":
        far = (face(G.x0, 0.6 * p.R_oa), face(G.y0, 0.6 * p.R_oa), face(G.z0, zhi - 20 * h))
        org = (face(G.x0, -0.6 * p.R_oa), face(G.y0, -0.6 * p.R_oa), face(G.z0, 20 * h))
    else:
        far = (face(G.x0, xhi - 12 * h), face(G.y0, xhi - 6 * h), face(G.z0, zhi - 20 * h))
        org = (face(G.x0, 12 * h), face(G.y0, 3 * h), face(G.z0, 20 * h))
    anchor = []
    q = 0
    for aname, A in (("far", far), ("origin", org)):
        k = 0
        for dname in DIRS:
            for sname, _ in _separations(cr):
                ctr = np.array(A, dtype=np.float64)
                # pairs of one anchor 3.1 cr apart along z (face and edge), corners two cells apart and three cells over in y
                if dname == "face":
                    ctr[1] += 0.41 * h
                    ctr[2] += (k - 10) * 3.1 * cr + 0.37 * h
                elif dname == "edge":
                    ctr[2] += (k - 10) * 3.1 * cr + 0.33 * h
                else:
                    ctr[1] += 3 * h
                    ctr[2] += (k - 17) * 2 * h
                i, j = _spread_indices(q, b.T, n)
                b.pair(i, j, ctr, dname, sname, f"{aname}_{dname}_{sname}")
                anchor.append(aname)
                k += 1
                q += 1
    ext = [G.gx * h, G.gy * h, G.gz * h]
    R2 = ext[0] * ext[0] + ext[1] * ext[1] + ext[2] * ext[2]
    margin = np.array([exact_margin(b.at[i], b.at[j], cr) for i, j in b.pairs])
    thr = cr * cr * CR2_INFLATE + 64.0 * 2.0 ** -53 * R2
    return b.finish(dict(band=2.0 ** -53 * R2, margin=margin, anchor=anchor, thr=thr, origin=(G.x0, G.y0, G.z0)))


# ---------------------------------------------------------------------------------------------------------- outside the grid
def outside(kind="pore", n=16 * AP2_T + 544):
    """The pairs of edge_states.outside_pairs — below z = 0, beyond R_oa and above H, by less and by more than one grid cell —
    among fillers up to n >= 16384, for a sweep run BEFORE walls and bounds: the tiled kernel sees coordinates outside the
    extent its error bound is computed from.  Here ``collide`` is the overlap alone (every pair overlaps); whether a pair is
    hit is decided by its membership of a reference cell, which is the oracle's to say: hits > 0 implies collide."""
    assert kind == "pore" and n >= SWITCH_N
    b = _Build(kind, n, landed=False)
    p, cr = b.p, b.cr
    h = FINE_MULT * cr
    spots = [(1e-9, 2e-9, -0.3 * cr), (4e-9, 2e-9, -0.6 * h), (8e-9, 2e-9, -1.5 * h), (p.R_oa + 0.2 * cr, 0.0, 0.5 * p.h_oa),
             (0.0, p.R_oa + 2.5 * h, 0.3 * p.h_oa), (1.5e-8, 1.1e-8, p.H + 0.4 * cr), (-1.5e-8, 1.1e-8, p.H + 2.2 * h)]
    k = 0
    for q, (x, y, z) in enumerate(spots):
        for w, m in enumerate((1, 0)):
            sep = cr * (1.0 - m * 2.0 ** -52) if m else cr * 0.5
            a = np.array([x, y + 4 * cr * w, z])
            e = np.array([0.0, 0.0, sep]) if q < 3 or q >= 5 else np.array([sep, 0.0, 0.0])
            i, j = _spread_indices(k, b.T, n)
            # (pair() straddles a centre along x: place the two by hand, as outside_pairs does)
            b._put(j, f"outside_{q}", a, (0.0, 5.0, 80.0), a)
            b._put(i, f"outside_{q}", a + e, (0.0, 5.0, -80.0), a + e)
            b._record(i, j, "in_1" if m else "half", None)
            k += 1
    return b.finish()


# ---------------------------------------------------------------------------------------------------------- judging a run
def pair_hits(rec, pairs):
    """per crafted pair: how many times the completed-path records show a collision between its two particles (every
    particle starts with its flag set); and the set of particle indices in any record"""
    pp = rec[rec["j"] >= 0]
    key = np.minimum(pp["i"], pp["j"]).astype(np.int64) * (1 << 32) + np.maximum(pp["i"], pp["j"])
    key = key[pp["which"] == 0]
    want = np.minimum(pairs[:, 0], pairs[:, 1]) * (1 << 32) + np.maximum(pairs[:, 0], pairs[:, 1])
    hits = np.array([(key == w).sum() for w in want])
    seen = set(rec["i"].tolist()) | set(pp["j"].tolist())
    return hits, seen


# ---------------------------------------------------------------------------------------------------------- the expanded form
def _fl(v):
    return float(v)                     # (Fraction -> float rounds to nearest even: one IEEE operation)


def _fma(a, b, c):
    return _fl(Fraction(a) * Fraction(b) + Fraction(c))


def tiled_test(ri, rj, origin, thr):
    """k_detect_allpairs_tiled's test of one pair, operation by operation: coordinates relative to the grid origin, the
    squared norms by one product and two fused multiply-adds, t = |rj|^2 - 2 ri.rj by three fused multiply-adds against
    thr - |ri|^2.  Returns (passes, t - (thr - |ri|^2) as the kernel holds the two)."""
    X, Y, Z = (float(ri[k]) - origin[k] for k in range(3))
    jx, jy, jz = (float(rj[k]) - origin[k] for k in range(3))
    ti = thr - _fma(Z, Z, _fma(Y, Y, X * X))
    jn = _fma(jz, jz, _fma(jy, jy, jx * jx))
    t = _fma(-2.0 * Z, jz, _fma(-2.0 * Y, jy, _fma(-2.0 * X, jx, jn)))
    return t < ti, t - ti
