"""GPU (-m gpu): the overlap removal of a synthetic start (include/argonmc-ic.h) against its host mirror (tests/ic_separate_ref.py).
In the cube the whole loop is compared bit for bit (every operation of the recipe is one IEEE product); in the pore the device's
cos, sin and sqrt differ from libm in the last place, so the loop is followed round by round from the downloaded doubles.  The
crafted states use exact coordinates: whole multiples of U = 2^-32 m with min_dist = 3 U, so that every square and sum is exact
and 8 < 9 overlaps while 9 < 9 does not."""
import math

import numpy as np
import pytest

from argon_monte_carlo_amd import ic as IC
from argon_monte_carlo_amd import params as PR
from tests import ic_separate_ref as REF

pytestmark = pytest.mark.gpu

U = 2.0 ** -32
FIELDS = ("x", "y", "z", "vx", "vy", "vz", "d", "dx", "dy", "dz", "flag")
REST = FIELDS[3:]
AMC_ERR_INVALID, AMC_ERR_CAPACITY, AMC_ERR_STATE = -1, -4, -6


def _cube(n, factor=1, seed=1):
    p, c = PR.cube_params_for_n(n, sigma=factor * PR.SIGMA)
    return p, c, IC.device_ic_config(p, c, seed, "cube"), (p.cube_x, p.cube_y, p.cube_z)


def _pore(seed=17, energised=False):
    p, c = PR.pore_params(n=8000, sigma=100 * PR.SIGMA, energised=energised)
    return p, c, IC.device_ic_config(p, c, seed, "pore"), (p.cube_x, p.cube_y, p.cube_z)


def _engine(p, cfg=None):
    from argon_monte_carlo_amd.engine import Engine
    eng = Engine(p)
    if cfg is not None:
        eng.init_synthetic(cfg)
    return eng


def _xyz(s):
    return s["x"], s["y"], s["z"]


def _same(a, b, keys=FIELDS, ctx=""):
    for k in keys:
        assert np.array_equal(a[k], b[k]), (ctx, k, np.flatnonzero(a[k] != b[k])[:5])


_MADE = {}


def _plain(name):
    """(p, c, cfg, cube, the plain init's download) of the named case, made once and never changed"""
    if name not in _MADE:
        p, c, cfg, cube = {"cube4096": lambda: _cube(4096, 16, 12345), "cube1000": lambda: _cube(1000, 36, 7), "pore": lambda: _pore(),
                           "temp": lambda: _pore(energised=True)}[name]()
        eng = _engine(p, cfg)
        _MADE[name] = (p, c, cfg, cube, eng.download())
        eng.close()
    return _MADE[name]


def _mirror(name, **kw):
    """the mirror's loop from the plain init's download, once per (case, arguments)"""
    key = (name, tuple(sorted(kw.items())))
    if key not in _MADE:
        p, c, cfg, cube, plain = _plain(name)
        _MADE[key] = REF.separate(*_xyz(plain), cfg, cube, p.collision_range, **kw)
    return _MADE[key]


# ---- 1. the cube, bit for bit -------------------------------------------------------------------------------------------------------
def test_cube_equals_the_mirror_bit_for_bit():
    p, c, cfg, cube, plain = _plain("cube4096")
    for a, b in zip(_xyz(plain), REF.initial_positions(cfg, cube, 4096)):
        assert np.array_equal(a, b)                 # (round 0 is the generator's own recipe)
    X, Y, Z, want = _mirror("cube4096")
    assert want["pairs_first"] > 400 and want["rounds"] >= 3 and want["pairs_left"] == 0
    eng = _engine(p, cfg)
    st = eng.init_separate(cfg, p.collision_range)
    got = eng.download()
    eng.close()
    print(st)
    assert st == want
    assert np.array_equal(got["x"], X) and np.array_equal(got["y"], Y) and np.array_equal(got["z"], Z)
    _same(got, plain, REST)
    _, first = REF.search(*_xyz(plain), p.collision_range)
    moved = (got["x"] != plain["x"]) | (got["y"] != plain["y"]) | (got["z"] != plain["z"])
    assert moved[first].all() and st["losers_first"] <= moved.sum() <= st["redrawn"]
    mirror_moved = (X != plain["x"]) | (Y != plain["y"]) | (Z != plain["z"])
    assert np.array_equal(moved, mirror_moved)      # untouched atoms are bitwise the plain init's


# ---- 2. a spent budget, and its resume ----------------------------------------------------------------------------------------------
def test_a_spent_budget_leaves_pairs_and_resumes_bitwise():
    p, c, cfg, cube, plain = _plain("cube1000")
    full = _mirror("cube1000", max_rounds=64)
    part = _mirror("cube1000", max_rounds=3)
    assert full[3]["rounds"] > 3 and part[3]["pairs_left"] > 0
    one = _engine(p, cfg)
    st_one = one.init_separate(cfg, p.collision_range, max_rounds=64)
    two = _engine(p, cfg)
    st_a = two.init_separate(cfg, p.collision_range, max_rounds=3)
    mid = two.download()
    print(st_one, st_a)
    assert st_a == part[3] and st_a["next_round"] == 4 and st_a["pairs_left"] > 0
    for k, a in zip("xyz", part[:3]):
        assert np.array_equal(mid[k], a), k
    st_b = two.init_separate(cfg, p.collision_range, first_round=st_a["next_round"], max_rounds=64 - 3)
    assert st_one == full[3]
    _same(two.download(), one.download(), ctx="resumed")
    for k, a in zip("xyz", full[:3]):
        assert np.array_equal(one.download()[k], a), k
    assert st_b["next_round"] == st_one["next_round"] and st_a["redrawn"] + st_b["redrawn"] == st_one["redrawn"]
    assert st_b["pairs_first"] == st_a["pairs_left"] and st_b["pairs_left"] == 0
    one.close()
    two.close()


def test_a_query_changes_nothing_and_reports_the_counts():
    p, c, cfg, cube, plain = _plain("cube1000")
    eng = _engine(p, cfg)
    st = eng.init_separate(cfg, p.collision_range, max_rounds=0)
    pairs, losers = REF.search(*_xyz(plain), p.collision_range)
    assert st == dict(searches=1, rounds=0, redrawn=0, pairs_first=pairs, losers_first=len(losers), pairs_left=pairs, losers_left=len(losers),
                      next_round=1) and pairs > 0
    _same(eng.download(), plain)
    eng.close()


def test_separate_overlaps_raises_when_pairs_are_left():
    from argon_monte_carlo_amd._lib import ArgonMCError
    from argon_monte_carlo_amd.sim import Simulation
    p, c, cfg, cube, plain = _plain("cube1000")
    sim = Simulation("cube", params=p, consts=c)
    sim.init_synthetic(seed=7, device=True)
    assert np.array_equal(sim.x_vals, plain["x"])               # (the state cache is filled here ...)
    with pytest.raises(ArgonMCError) as e:
        sim.separate_overlaps(max_rounds=3)
    part = _mirror("cube1000", max_rounds=3)
    assert e.value.code == AMC_ERR_CAPACITY and str(part[3]["pairs_left"]) in str(e.value) and str(part[3]["losers_left"]) in str(e.value)
    assert np.array_equal(sim.x_vals, part[0])                  # (... and dropped: the state is the last round's)
    # the keyword of init_synthetic, behind the device generator and behind the host one
    sim.init_synthetic(seed=7, device=True, separate=True)
    assert np.array_equal(sim.x_vals, _mirror("cube1000", max_rounds=64)[0])
    sim.init_synthetic(seed=7, separate=True)
    assert REF.search(sim.x_vals, sim.y_vals, sim.z_vals, p.collision_range)[0] == 0
    host = IC.cube_ic(p, c, 7)
    assert REF.search(*host[:3], p.collision_range)[0] > 0 and np.array_equal(sim.x_velocities, host[3])
    sim.init_synthetic(seed=7)                                  # the default is unchanged
    assert np.array_equal(sim.x_vals, host[0])
    sim.close()


# ---- 3. the pore, round by round ----------------------------------------------------------------------------------------------------
def _in_region(cfg, j, x, y, z):
    r = REF.region_index(cfg, j)
    return math.hypot(x, y) <= float(cfg.radius[r]) * (1 + 1e-12) and float(cfg.z_lo[r]) <= z <= float(cfg.z_hi[r])


def _round_by_round(eng, p, cfg, cube, plain, budget=16):
    state, t = plain, 1
    while True:
        pairs, losers = REF.search(*_xyz(state), p.collision_range)
        if pairs == 0:
            break
        assert t <= budget
        st = eng.init_separate(cfg, p.collision_range, first_round=t, max_rounds=1)
        assert (st["pairs_first"], st["losers_first"], st["rounds"], st["redrawn"], st["next_round"]) == (pairs, len(losers), 1, len(losers), t + 1)
        new = eng.download()
        moved = (new["x"] != state["x"]) | (new["y"] != state["y"]) | (new["z"] != state["z"])
        assert np.array_equal(np.flatnonzero(moved), losers), t          # exactly the losers changed
        _same(new, plain, REST, t)
        for j in losers:
            want = REF.position(cfg, cube, int(j), t)
            got = (new["x"][j], new["y"][j], new["z"][j])
            assert _in_region(cfg, int(j), *got), (t, j)
            assert np.allclose(got, want, rtol=1e-12, atol=0.0), (t, j, got, want)
        state, t = new, t + 1
    st = eng.init_separate(cfg, p.collision_range, first_round=t, max_rounds=1)
    assert (st["searches"], st["rounds"], st["pairs_first"], st["pairs_left"], st["next_round"]) == (1, 0, 0, 0, t)
    _same(eng.download(), state)
    return state, t - 1


@pytest.mark.parametrize("name", ["pore", "temp"])
def test_pore_round_by_round(name):
    p, c, cfg, cube, plain = _plain(name)
    want = _mirror(name)[3]
    pairs, losers = REF.search(*_xyz(plain), p.collision_range)
    assert pairs > 100 and (pairs, len(losers)) == (want["pairs_first"], want["losers_first"])     # (libm's last place moves no pair here)
    if name == "temp":
        from argon_monte_carlo_amd.sim import TemperatureSimulation
        sim = TemperatureSimulation(params=p, consts=c, device_rng_seed=5)
        sim.init_synthetic(seed=17, device=True)
        eng = sim.engine
        _same(eng.download(), plain)
    else:
        eng = _engine(p, cfg)
    final, rounds = _round_by_round(eng, p, cfg, cube, plain)
    assert rounds >= 2
    assert REF.search(*_xyz(final), p.collision_range)[0] == 0
    for first, end, R, zl, zh in REF.regions_of(cfg):
        s = slice(first, end)
        assert (np.hypot(final["x"][s], final["y"][s]) <= R * (1 + 1e-12)).all() and (final["z"][s] >= zl).all() and (final["z"][s] <= zh).all()
    if name == "temp":
        # the driver's own call, from the plain init again: the same state as the rounds one by one
        sim.init_synthetic(seed=17, device=True)
        st = sim.separate_overlaps()
        assert st["rounds"] == rounds and st["pairs_left"] == 0
        _same(eng.download(), final)
        sim.run(2)
        sim.close()
    else:
        eng.close()


# ---- 4. crafted states --------------------------------------------------------------------------------------------------------------
class Crafted:
    """Groups of atoms on whole multiples of U in a cube, each group alone in its neighbourhood of cells: the expected pairs and
    losers add up group by group.  `cells`, `w`: the library's own search cells for min_dist = 3 U at the default knob."""

    def __init__(self, L):
        self.L = L
        edge = 3 * U * (1.0 + 2.0 ** -20)
        self.cells = int(min(max(math.floor(L / edge), 1), 128))
        self.w = L / self.cells
        self.pos, self.pairs, self.losers, self.group = [], 0, [], 0

    def cell(self, m):
        f = math.floor((m * U - 0.0) / self.w)
        return int(min(max(f, 0), self.cells - 1))

    def find(self, d, cross, start, span=16):
        """the lowest whole a >= start whose cell and that of a + d differ (cross) or do not"""
        a = start
        while (self.cell(a) != self.cell(a + d)) != bool(cross):
            a += 1
            assert a < start + span, (d, cross, start)
        return a

    def anchor(self):
        """whole coordinates of the low corner region of the next group's own cells: five cells apart on a lattice"""
        per = (self.cells - 3) // 5
        g, self.group = self.group, self.group + 1
        assert g < per ** 3
        c = [1 + 5 * (g % per), 1 + 5 * ((g // per) % per), 1 + 5 * (g // (per * per))]
        return [int(math.ceil(k * self.w / U)) + 1 for k in c]

    def add(self, atoms, pairs, losers):
        """atoms: whole coordinates; losers: positions within `atoms`"""
        base = len(self.pos)
        self.pos += [tuple(a) for a in atoms]
        self.pairs += pairs
        self.losers += [base + k for k in losers]

    def pair(self, off, cross, a0=None, span=16):
        """two atoms `off` apart, crossing a cell boundary on exactly the axes of `cross`"""
        a0 = self.anchor() if a0 is None else a0
        a = [self.find(off[k], cross[k], a0[k], span) for k in range(3)]
        for k in range(3):
            assert (self.cell(a[k]) != self.cell(a[k] + off[k])) == bool(cross[k])
        hit = off[0] ** 2 + off[1] ** 2 + off[2] ** 2 < 9
        self.add([a, [a[k] + off[k] for k in range(3)]], int(hit), [1] if hit else [])

    def arrays(self):
        a = np.array(self.pos, dtype=np.float64) * U
        return a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy()


def _perm(off, axes):
    """`off` with its nonzero components (largest first) on `axes` and zeros elsewhere"""
    out, vals = [0, 0, 0], sorted((v for v in off if v), reverse=True)
    assert len(vals) >= len(axes)
    rest = [k for k in range(3) if k not in axes]
    for k, v in zip(list(axes) + rest, vals):
        out[k] = v
    return out


def _crafted(L):
    s = Crafted(L)
    # 8 < 9 overlaps; 9 < 9 does not: inside one cell, across a face on each axis, across an edge, across a corner — wherever the
    # offset has a component on every axis that is crossed ((2, 2, 0) and (3, 0, 0) cannot straddle a corner, (3, 0, 0) no edge:
    # there (2, 1, 1), 6 < 9, stands in for the overlapping pair)
    for off in ((2, 2, 0), (2, 2, 1), (3, 0, 0), (2, 1, 1)):
        if off == (3, 0, 0):
            # (a cell barely wider than 3 U holds four whole coordinates only here and there: anywhere along a row of cells that
            # no other group comes near, the highest of the lattice)
            top = int(math.ceil((s.cells - 4) * s.w / U)) + 1
            s.pair(off, (0, 0, 0), a0=[5, top, top], span=int(L / U) - 12)
        else:
            s.pair(_perm(off, (0,)), (0, 0, 0))
        for ax in range(3):
            s.pair(_perm(off, (ax,)), [int(k == ax) for k in range(3)])
        if sum(1 for v in off if v) >= 2:
            for axes in ((0, 1), (0, 2), (1, 2)):
                s.pair(_perm(off, axes), [int(k in axes) for k in range(3)])
        if sum(1 for v in off if v) == 3:
            s.pair(off, (1, 1, 1))
    # the same pairs mirrored (negative offsets: the higher index sits in the lower cell)
    s.pair((-2, -2, 0), (1, 1, 0))
    s.pair((-2, -2, -1), (1, 1, 1))
    # the box's first and last cells, and atoms outside the box on either side: the clamp
    m = int(math.floor(L / U))
    s.add([(1, 1, 1), (3, 3, 1)], 1, [1])
    s.add([(m - 1, m - 1, m - 1), (m - 3, m - 3, m - 1)], 1, [1])
    s.add([(-5, -5, -5), (-3, -3, -5)], 1, [1])                     # both outside, below
    s.add([(m + 9, m + 9, m + 9), (m + 11, m + 11, m + 9)], 1, [1])     # both outside, beyond
    s.add([(-1, 20, 20), (1, 22, 20)], 1, [1])                      # one outside, one inside
    s.add([(40, m + 1, 20), (42, m - 1, 20)], 1, [1])
    s.add([(-1000, 40, 40), (-1000, 40, 43)], 0, [])                # far outside, not overlapping, in one clamped cell
    s.add([(60, 60, -4000), (60, 62, -4002)], 1, [1])
    # a chain i < j < k, in the three orders of its middle atom
    a = s.anchor()
    s.add([(a[0], a[1], a[2]), (a[0] + 2, a[1], a[2]), (a[0] + 4, a[1], a[2])], 2, [1, 2])
    a = s.anchor()
    s.add([(a[0] + 2, a[1], a[2]), (a[0], a[1], a[2]), (a[0] + 4, a[1], a[2])], 2, [1, 2])
    a = s.anchor()
    s.add([(a[0], a[1], a[2]), (a[0] + 4, a[1], a[2]), (a[0] + 2, a[1], a[2])], 2, [2])
    # one atom over five of a lower index that keep clear of each other: five pairs, one loser
    a = s.anchor()
    a = [v + 2 for v in a]
    s.add([(a[0] + 2, a[1] + 2, a[2]), (a[0] - 2, a[1] - 2, a[2]), (a[0] + 2, a[1] - 2, a[2]), (a[0] - 2, a[1] + 2, a[2]), (a[0], a[1], a[2] + 2),
           (a[0], a[1], a[2])], 5, [5])
    # home cells of 1, 64, 65 and 129 atoms (the tile's edges): k atoms at one point, and a neighbour of a higher index (2, 2, 0)
    # away across a face that overlaps them all
    for k in (1, 64, 65, 129):
        a0 = s.anchor()
        a = [s.find(2, 1, a0[0]), s.find(2, 0, a0[1]), a0[2]]
        s.add([a] * k + [(a[0] + 2, a[1] + 2, a[2])], k * (k - 1) // 2 + k, list(range(1, k + 1)))
    return s


@pytest.mark.parametrize("cells", [None, "16", "1"])
def test_crafted_pairs_at_the_rules_and_the_cells_edges(cells, monkeypatch):
    if cells is not None:
        monkeypatch.setenv("AMC_IC_CELLS", cells)
    n = len(_crafted(_cube(330)[0].cube_x).pos)
    p, c, cfg, cube = _cube(n)
    s = _crafted(p.cube_x)
    assert len(s.pos) == n and s.cells >= 28
    x, y, z = s.arrays()
    assert len(set(s.pos)) < n and (x / U == np.round(x / U)).all()
    # the mirror and brute force agree with the hand count
    pairs, losers = REF.brute_search(x, y, z, 3 * U)
    assert pairs == s.pairs and list(losers) == sorted(s.losers)
    pairs, losers = REF.search(x, y, z, 3 * U)
    assert pairs == s.pairs and list(losers) == sorted(s.losers)
    eng = _engine(p)
    rest = [np.arange(n) * 1.0 + k for k in range(7)]
    eng.upload(x, y, z, *rest, flag=np.arange(n) % 2)
    before = eng.download()
    st = eng.init_separate(cfg, 3 * U, max_rounds=0)
    assert (st["pairs_first"], st["losers_first"], st["pairs_left"], st["searches"]) == (s.pairs, len(s.losers), s.pairs, 1)
    _same(eng.download(), before)
    st = eng.init_separate(cfg, 3 * U, max_rounds=1)
    after = eng.download()
    moved = (after["x"] != x) | (after["y"] != y) | (after["z"] != z)
    assert np.array_equal(np.flatnonzero(moved), sorted(s.losers)) and st["redrawn"] == len(s.losers) and st["rounds"] == 1
    _same(after, before, REST)
    for j in s.losers:
        assert (after["x"][j], after["y"][j], after["z"][j]) == REF.position(cfg, cube, j, 1)
    X, Y, Z, want = REF.separate(x, y, z, cfg, cube, 3 * U, max_rounds=1)
    assert st == want
    eng.close()


def test_first_and_last_index_of_every_region_keep_to_their_cylinder():
    p, c, cfg, cube, plain = _plain("pore")
    regions = REF.regions_of(cfg)
    x, y, z = (plain[k].copy() for k in "xyz")
    ends = []
    for r, (first, end, R, zl, zh) in enumerate(regions):
        # the last atom of the region onto atom 1 (region 0), the first one onto the atom in front of it (the region before)
        for j, onto in ((end - 1, 1), (first, first - 1)):
            if j > 1 and onto >= 0:
                x[j], y[j], z[j] = x[onto], y[onto], z[onto]
                ends.append(j)
    assert len(ends) == 9
    eng = _engine(p)
    eng.upload(x, y, z, *[plain[k] for k in REST[:-1]], flag=plain["flag"])
    pairs, losers = REF.search(x, y, z, p.collision_range)
    assert set(ends) <= set(losers)
    st = eng.init_separate(cfg, p.collision_range, max_rounds=1)
    assert (st["pairs_first"], st["losers_first"]) == (pairs, len(losers))
    new = eng.download()
    for j in ends:
        got = (new["x"][j], new["y"][j], new["z"][j])
        assert _in_region(cfg, j, *got), j
        assert np.allclose(got, REF.position(cfg, cube, j, 1), rtol=1e-12, atol=0.0), j
    eng.close()


def test_everybody_at_one_point():
    p, c, cfg, cube = _cube(4096, seed=3)
    eng = _engine(p, cfg)
    plain = eng.download()
    m = float(round(0.4 * p.cube_x / U)) * U
    pt = np.full(4096, m)
    eng.upload(pt, pt, pt, *[plain[k] for k in REST[:-1]], flag=plain["flag"])
    st = eng.init_separate(cfg, 3 * U, max_rounds=0)
    assert (st["pairs_first"], st["losers_first"]) == (8386560, 4095) == (4096 * 4095 // 2, 4095)
    # ... and apart again: atom 0 stays, everybody else is redrawn, and the loop ends as the mirror's does
    st = eng.init_separate(cfg, 3 * U)
    X, Y, Z, want = REF.separate(pt, pt, pt, cfg, cube, 3 * U)
    got = eng.download()
    assert st == want and st["pairs_left"] == 0 and st["redrawn"] >= 4095
    assert np.array_equal(got["x"], X) and np.array_equal(got["y"], Y) and np.array_equal(got["z"], Z) and got["x"][0] == m
    eng.close()


# ---- 5. independence of the grid and the launch -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cube4096", "pore"])
def test_the_cell_knob_changes_nothing(name, monkeypatch):
    p, c, cfg, cube, plain = _plain(name)
    ref = None
    for cells in (None, "1", "3", "7"):
        if cells is None:
            monkeypatch.delenv("AMC_IC_CELLS", raising=False)
        else:
            monkeypatch.setenv("AMC_IC_CELLS", cells)
        eng = _engine(p, cfg)
        st = eng.init_separate(cfg, p.collision_range)
        got = eng.download()
        eng.close()
        if ref is None:
            ref = (st, got)
            assert st["pairs_first"] > 100 and st["pairs_left"] == 0
        else:
            assert st == ref[0], cells
            _same(got, ref[1], ctx=cells)


# ---- 6. shards ----------------------------------------------------------------------------------------------------------------------
def test_two_shards_hold_the_single_contexts_system():
    from argon_monte_carlo_amd.engine import ShardEngine
    p, c, cfg, cube, plain = _plain("cube4096")
    X, Y, Z, want = _mirror("cube4096")
    states, stats = [], []
    for lo, hi in ((0, 4096), (0, 1501), (1501, 4096)):
        eng = ShardEngine(p, lo, hi)
        eng.init_synthetic(cfg)
        a = eng.init_separate(cfg, p.collision_range, max_rounds=2)
        b = eng.init_separate(cfg, p.collision_range, first_round=a["next_round"])
        assert a["pairs_left"] > 0 and b["pairs_left"] == 0 and a["redrawn"] + b["redrawn"] == want["redrawn"] and b["next_round"] == want["next_round"]
        states.append(eng.download())
        stats.append((a, b))
        eng.close()
    assert stats[0] == stats[1] == stats[2]
    _same(states[0], states[2])
    _same(states[0], states[1])
    assert np.array_equal(states[0]["x"], X) and np.array_equal(states[0]["y"], Y) and np.array_equal(states[0]["z"], Z)
    _same(states[0], plain, REST)


def test_the_sharded_driver_passes_through():
    from argon_monte_carlo_amd.dist import ShardedSimulation
    p, c, cfg, cube, plain = _plain("cube4096")
    X, Y, Z, want = _mirror("cube4096")

    class NoComm:
        shortcut = True

    from argon_monte_carlo_amd.engine import ShardEngine
    sim = ShardedSimulation(p, 0, 1, engine=ShardEngine(p, 0, 4096), comm=NoComm())
    sim.init_synthetic(cfg)
    assert sim.init_separate(cfg, p.collision_range) == want
    got = sim.engine.download()
    assert np.array_equal(got["x"], X) and np.array_equal(got["z"], Z)
    sim.engine.close()


# ---- 7. usable and effective --------------------------------------------------------------------------------------------------------
def test_the_separated_state_runs_like_the_oracles():
    from oracle import oracle as O
    p, c, cfg, cube, plain = _plain("cube4096")
    eng = _engine(p, cfg)
    eng.init_separate(cfg, p.collision_range)
    start = eng.download()
    orc = O.Oracle(p, mode="mul")
    orc.upload(*[start[k] for k in FIELDS[:10]], flag=start["flag"])
    first = None
    for q in range(5):
        st = eng.timestep(c["dt"])
        rc, so = orc.timestep(c["dt"])
        assert rc == 0 and st["flags"] == 0 and st["n_pp"] == so["n_pp"], (q, st, so)
        first = st if first is None else first
    dev, ref = eng.download(), orc.state()
    for k in FIELDS[:10]:
        assert np.array_equal(dev[k], ref[k]), k
    eng.close()
    raw = _engine(p, cfg)
    st_plain = raw.timestep(c["dt"])
    raw.close()
    print("step 1 n_pp: separated %d, plain %d" % (first["n_pp"], st_plain["n_pp"]))
    assert first["n_pp"] < st_plain["n_pp"]


def test_the_pair_sampler_finds_no_overlap_afterwards():
    from argon_monte_carlo_amd.sim import Simulation
    p, c, cfg, cube, plain = _plain("cube4096")
    sim = Simulation("cube", params=p, consts=c)
    sim.enable_pairs()
    sim.init_synthetic(seed=12345, device=True)
    sim.pairs_sample()
    before = sim.pairs()["overlap_per_centre"]
    assert np.isfinite(before).all() and (before >= 0).all() and before.sum() > 0
    sim.pairs_reset()
    sim.separate_overlaps(min_dist=1.001 * p.collision_range)
    sim.pairs_sample()
    after = sim.pairs()["overlap_per_centre"]
    assert np.isfinite(after).all() and (after == 0).all(), after
    sim.close()


# ---- 8. ownership, the empty systems, what the call refuses -------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2])
def test_the_smallest_systems(n):
    p, c, cfg, cube = _cube(n, seed=5)
    eng = _engine(p, cfg)
    owned = eng.owned_count()
    st = eng.init_separate(cfg, 1e-3)               # (further than the cube is wide: two atoms never come apart)
    assert eng.owned_count() == owned
    if n < 2:
        assert st == dict(searches=1, rounds=0, redrawn=0, pairs_first=0, losers_first=0, pairs_left=0, losers_left=0, next_round=1)
    else:
        assert st == dict(searches=65, rounds=64, redrawn=64, pairs_first=1, losers_first=1, pairs_left=1, losers_left=1, next_round=65)
        got = eng.download()
        assert (got["x"][1], got["y"][1], got["z"][1]) == REF.position(cfg, cube, 1, 64)
        assert (got["x"][0], got["y"][0], got["z"][0]) == REF.position(cfg, cube, 0, 0)
    assert eng.init_separate(cfg, 1e-3, first_round=7, max_rounds=0)["next_round"] == 7
    eng.run(c["dt"], 2)
    eng.close()


def test_ownership_with_every_sampler_and_a_pending_result():
    from argon_monte_carlo_amd.sim import TemperatureSimulation
    p, c, cfg, cube, plain = _plain("temp")
    sim = TemperatureSimulation(params=p, consts=c, device_rng_seed=5)
    sim.enable_fields(every=1)
    sim.enable_correlations(every=1)
    sim.enable_fluxes(every=1)
    sim.enable_free_paths()
    sim.enable_distributions(every=1)
    sim.enable_transits()
    sim.enable_pairs(every=2)
    sim.enable_surface()
    sim.init_synthetic(seed=17, device=True)
    eng = sim.engine
    owned = eng.owned_count()
    st = sim.separate_overlaps()
    assert eng.owned_count() == owned and st["pairs_left"] == 0 and st["rounds"] >= 2
    sim.timestep()                                  # a step's deferred results are pending behind it
    owned = eng.owned_count()
    assert eng.init_separate(cfg, p.collision_range, max_rounds=0)["rounds"] == 0
    st = eng.init_separate(cfg, 3 * p.collision_range, max_rounds=2)
    assert eng.owned_count() == owned and st["rounds"] >= 1
    sim.run(3)
    assert sim.pairs()["n_samples"] >= 1
    sim.close()


def test_what_the_call_refuses():
    from argon_monte_carlo_amd._lib import ArgonMCError
    p, c, cfg, cube, plain = _plain("cube1000")
    eng = _engine(p)

    def code(*a, e=eng, g=cfg, **kw):
        with pytest.raises(ArgonMCError) as err:
            e.init_separate(g, *a, **kw)
        return err.value.code

    assert code(p.collision_range) == AMC_ERR_STATE                 # no state yet
    eng.init_synthetic(cfg)
    owned = eng.owned_count()
    for bad in (0.0, -1e-9, math.inf, -math.inf, math.nan):
        assert code(bad) == AMC_ERR_INVALID, bad
    assert code(p.collision_range, first_round=0) == AMC_ERR_INVALID
    assert code(p.collision_range, first_round=-3) == AMC_ERR_INVALID
    assert code(p.collision_range, max_rounds=-1) == AMC_ERR_INVALID
    assert code(p.collision_range, first_round=2 ** 31 - 1, max_rounds=1) == AMC_ERR_INVALID
    assert code(p.collision_range, first_round=2 ** 30, max_rounds=2 ** 30) == AMC_ERR_INVALID
    bad = IC.device_ic_config(p, c, 7, "cube")
    bad.n_regions = 9
    assert code(p.collision_range, g=bad) == AMC_ERR_INVALID
    bad = IC.device_ic_config(p, c, 7, "cube")
    bad.struct_size = 8
    assert code(p.collision_range, g=bad) == AMC_ERR_INVALID
    pp, pc, pcfg, _ = _pore()
    assert code(p.collision_range, g=pcfg) == AMC_ERR_INVALID       # the regions hold another number of atoms
    _same(eng.download(), plain)
    # at the limit of the round counter the query still runs; a_shape is ignored
    ok = IC.device_ic_config(p, c, 7, "cube")
    ok.a_shape = -1.0
    assert eng.init_separate(ok, p.collision_range, first_round=2 ** 31 - 1, max_rounds=0)["next_round"] == 2 ** 31 - 1
    assert eng.owned_count() == owned
    eng.close()
    pore = _engine(pp, pcfg)
    assert code(pp.collision_range, e=pore, g=IC.device_ic_config(pp, pc, 17, "cube")) == AMC_ERR_INVALID      # a pore needs the region table
    pore.close()
