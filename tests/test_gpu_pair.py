"""GPU (-m gpu): the sampled pair distribution (include/argonmc_pair.h).  Every comparison is exact integer equality against the
brute-force NumPy mirror (tests/pair_ref.py) on the state download() returns after the sample: crafted edges, the cell structure
at its limits, deferred sweep results, any launch geometry, the life cycle, the energised run and index-range shards."""
import math

import numpy as np
import pytest
import torch                # (first: the library then shares torch's HIP runtime — the three ranks exchange through torch)

from argon_monte_carlo_amd import ic as IC
from argon_monte_carlo_amd import pairs as PA
from argon_monte_carlo_amd import params as PR
from tests import fields_ref as FREF
from tests import pair_ref as REF
from tests.sampler_protocol import KEYS, make_temp_sim
from tests.sampler_protocol import PairMirror as Totals

pytestmark = pytest.mark.gpu

U = 2.0 ** -26                          # 14.9 nm: the crafted states' unit, exact in fp64 (the default cube is 100 nm = 6.71 U wide)


def _crafted(points, grid_of, lo=None, hi=None):
    """An engine over a cube context holding exactly ``points`` (rows x y z vx vy vz), its grid from ``grid_of(params)`` and one
    sample taken: (engine, grid, state, totals of the mirror)."""
    from argon_monte_carlo_amd.engine import Engine, ShardEngine
    pts = np.asarray(points, dtype=np.float64)
    p, _ = PR.cube_params(n=len(pts))
    eng = Engine(p) if lo is None else ShardEngine(p, lo, hi)
    state = tuple(pts[:, k].copy() for k in range(6))
    eng.upload(*state)
    eng.pair_config(grid_of(p))
    eng.pair_sample()
    ref = Totals(eng.pair_grid)
    ref.add_state(eng.download(), 0 if lo is None else lo, hi)
    return eng, eng.pair_grid, state, ref


def _cube_grid(r_max, hist_bins, n=(1, 1, 1)):
    return lambda p: PA.make_grid("cartesian", n, (0.0, 0.0, 0.0), (p.cube_x, p.cube_y, p.cube_z), r_max, hist_bins=hist_bins)


def _cells(g, x, y, z):
    """linear cell per particle as the device files it, -1 unfiled"""
    lo, hi, cells, edge = PA.search_box(g)
    c = [FREF._axis(np.asarray(u, dtype=np.float64), lo[a], hi[a], edge[a], cells[a]) for a, u in enumerate((x, y, z))]
    return np.where((c[0] >= 0) & (c[1] >= 0) & (c[2] >= 0), (c[0] * cells[1] + c[1]) * cells[2] + c[2], -1)


# ---- 1. crafted edges: the expected table is written out by hand ---------------------------------------------------------------
def test_crafted_pairs_land_in_the_documented_columns():
    """r_max = U, H = 8 (columns of U / 8).  Every pair sits on a line of its own, 2 U from the next one, with one end at x = 0 (on
    the grid's lower edge: inside), so every distance is exact."""
    below = float(np.nextafter(U, 0.0))
    pts, line = [], iter([(a * 2 * U + U / 2, b * 2 * U + U / 2) for a in range(3) for b in range(3)])

    def pair(r, vi=(0, 0, 0), vj=(0, 0, 0), xi=0.0):
        y, z = next(line)
        pts.append((xi, y, z) + tuple(vi))
        pts.append((xi + r, y, z) + tuple(vj))
    pair(U)                                     # 0, 1: exactly r_max: not counted
    pair(below)                                 # 2, 3: the last column, at rest: not approaching
    pair(3 * U / 8)                             # 4, 5: exactly on the edge between columns 2 and 3: column 3
    pair(0.0, xi=U, vi=(5, 0, 0), vj=(-5, 0, 0))    # 6, 7: coincident: column 0; dx = 0 makes s = 0: not approaching
    pair(U / 2, vi=(7, -3, 2), vj=(7, -3, 2))   # 8, 9: equal velocities: s = 0 is not approaching; column 4
    pair(U / 2, vi=(1, 0, 0), vj=(math.nan, 0, 0))   # 10, 11: a NaN velocity: counted, never approaching
    pair(U / 4, vi=(1, 0, 0), vj=(0, 0, 0))     # 12, 13: i runs into j: approaching, column 2
    pair(U / 4, vi=(-1, 0, 0), vj=(0, 0, 0))    # 14, 15: receding
    eng, g, state, ref = _crafted(pts, _cube_grid(U, 8))
    want = np.zeros((1, 17), dtype=np.int64)
    want[0, 0] = 16
    for col, approaching in ((7, 0), (3, 0), (0, 0), (4, 0), (4, 0), (2, 2), (2, 0)):
        want[0, 1 + col] += 2
        want[0, 9 + col] += approaching
    tot = ref.check(eng)
    assert np.array_equal(tot, want), np.argwhere(tot != want)
    assert (ref.n_outside, ref.n_unfiled) == (0, 0)
    eng.close()


def test_box_edge_outside_and_unfiled():
    """A partner outside the grid but inside the search box is a neighbour only and adds to n_outside; a particle outside the search
    box and one with a NaN position are unfiled and have no other effect."""
    y = z = 3 * U
    pts = [(0.0, y, z, 0, 0, 0),                # 0: a centre on the grid's face
           (-U / 2, y, z, 1, 0, 0),             # 1: outside the grid, inside the box: 0's neighbour, approaching it
           (-1.5 * U, y, z, 0, 0, 0),           # 2: outside the box, U from particle 1 and 1.5 U from the centre: unfiled
           (math.nan, y, z, 0, 0, 0),           # 3: unfiled
           (U / 4, math.nan, z, 0, 0, 0),       # 4: unfiled, although x and z sit next to the centre
           (5 * U, y, z, 0, 0, 0)]              # 5: a centre without a neighbour
    eng, g, state, ref = _crafted(pts, _cube_grid(U, 8))
    tot = ref.check(eng)
    want = np.zeros((1, 17), dtype=np.int64)
    want[0, 0], want[0, 1 + 4], want[0, 9 + 4] = 2, 1, 1
    assert np.array_equal(tot, want) and (ref.n_outside, ref.n_unfiled) == (1, 3)
    eng.close()


def test_corner_one_partner_in_each_of_the_26_neighbouring_cells():
    """Particle 0 in the middle of its cell, one partner just across each face, edge and corner — all within r_max — and one two
    cells away, beyond r_max.  The context's range is particle 0 alone, so the table is its row: 26 pairs."""
    p, _ = PR.cube_params(n=28)
    g = _cube_grid(U, 8)(p)
    lo, hi, cells, edge = PA.search_box(g)
    assert cells == [8, 8, 8] and edge[0] > U
    c = [lo[a] + 3.5 * edge[a] for a in range(3)]
    step = [0.5 * edge[a] + 0.01 * U for a in range(3)]
    pts = [tuple(c) + (0, 0, 0)]
    for sx in (-1, 0, 1):
        for sy in (-1, 0, 1):
            for sz in (-1, 0, 1):
                if (sx, sy, sz) != (0, 0, 0):
                    pts.append((c[0] + sx * step[0], c[1] + sy * step[1], c[2] + sz * step[2], 0, 0, 0))
    pts.append((c[0] + 1.6 * edge[0], c[1], c[2], 0, 0, 0))
    a = np.array(pts)
    cell = _cells(g, a[:, 0], a[:, 1], a[:, 2])
    assert len(set(cell[:27].tolist())) == 27 and (cell >= 0).all()          # 27 different cells: the home cell and its 26 neighbours
    home = np.array(np.unravel_index(cell[0], cells))
    assert all(np.abs(np.array(np.unravel_index(k, cells)) - home).max() == 1 for k in cell[1:27])
    assert np.abs(np.array(np.unravel_index(cell[27], cells)) - home).max() == 2
    eng, g, state, ref = _crafted(pts, _cube_grid(U, 8), lo=0, hi=1)
    tot = ref.check(eng)
    assert tot[0, 0] == 1 and tot[0, 1:9].sum() == 26 and tot[0, 9:].sum() == 0
    eng.close()
    eng, g, state, ref = _crafted(pts, _cube_grid(U, 8))          # ... and everybody as a centre
    tot = ref.check(eng)
    assert tot[0, 0] == 28 and tot[0, 1:9].sum() > 52
    eng.close()


def test_full_cells_more_particles_than_a_tile():
    """300 particles in a ball of radius r_max / 4 — more than a wave's tile of 64 centres, more than one tile of neighbours — so
    each has 299 neighbours; a second such ball in the adjacent cell, near enough for pairs across the cell face."""
    p, _ = PR.cube_params(n=600)
    g = _cube_grid(U, 16)(p)
    lo, hi, cells, edge = PA.search_box(g)
    rng = np.random.RandomState(4)
    v = rng.normal(size=(600, 3))
    v *= (0.25 * U * rng.uniform(size=600) ** (1.0 / 3.0) / np.linalg.norm(v, axis=1))[:, None]
    centre = np.array([lo[a] + 3.5 * edge[a] for a in range(3)])
    pos = v + centre
    pos[300:, 2] += edge[2]
    pts = np.concatenate([pos, rng.normal(size=(600, 3)) * 300.0], axis=1)
    cell = _cells(g, pos[:, 0], pos[:, 1], pos[:, 2])
    assert len(set(cell[:300].tolist())) == 1 and len(set(cell[300:].tolist())) == 1 and cell[300] == cell[0] + 1
    eng, g, state, ref = _crafted(pts, _cube_grid(U, 16))
    tot = ref.check(eng)
    assert tot[0, 0] == 600 and tot[0, 1:17].sum() > 2 * 300 * 299 and not (tot[0, 1:] % 2).any()
    assert tot[0, 1:9].sum() == 2 * 300 * 299           # within r_max / 2: the pairs inside either ball and no others
    eng.close()


# ---- 2. few cells, and the cap --------------------------------------------------------------------------------------------------
def test_one_and_two_cells_on_an_axis_are_clipped_not_visited_twice():
    """A grid thin in z (one cell: the extent is 2 r_max and a little) and half an r_max wide in y (two cells)."""
    n = 400
    p, _ = PR.cube_params(n=n)
    rng = np.random.RandomState(6)
    x = rng.uniform(0.0, p.cube_x, n)
    y = rng.uniform(1.0 * U, 4.0 * U, n)
    z = np.where(np.arange(n) % 2 == 0, 3.0 * U, 3.0 * U + rng.uniform(-1.2, 1.2, n) * U)
    x[[0, 2, 4]], y[[0, 2, 4]] = 3.0 * U, 2.0 * U       # three coincident particles on the lower corner of the second grid below
    v = rng.normal(size=(3, n)) * 300.0

    def grid(p):
        return PA.make_grid("cartesian", (3, 1, 1), (0.0, 2.0 * U, 3.0 * U), (p.cube_x, 2.5 * U, 3.0 * U * (1.0 + 2.0 ** -30)), U, hist_bins=8)
    assert PA.search_box(grid(p))[2] == [8, 2, 1]
    eng, g, state, ref = _crafted(np.stack([x, y, z, v[0], v[1], v[2]], axis=1), grid)
    tot = ref.check(eng)
    assert tot[:, 0].sum() > 10 and tot[:, 1:9].sum() > 20 and ref.n_outside > 100 and ref.n_unfiled > 20
    eng.close()
    # one cell on every axis (a grid of 2^-30 r_max: the box is 2 r_max and a little): the home cell is its own only neighbour
    eps = 1.0 + 2.0 ** -30
    eng, g, state, ref = _crafted(np.stack([x, y, z, v[0], v[1], v[2]], axis=1),
                                  lambda p: PA.make_grid("cartesian", (1, 1, 1), (3 * U, 2 * U, 3 * U), (3 * U * eps, 2 * U * eps, 3 * U * eps), U, hist_bins=4))
    assert PA.search_box(g)[2] == [1, 1, 1]
    tot = ref.check(eng)
    assert tot[0, 0] == 3 and tot[0, 1] >= 6 and tot[0, 1:5].sum() > 30
    eng.close()


def test_cap_of_128_cells_per_axis():
    """extent / r_max = 202: 128 cells per axis with an edge of 1.58 r_max, two million cells, most of them empty; 2,000 particles in
    a box of ten r_max give every one several neighbours, the rest is spread over the cube."""
    n = 2400
    p, _ = PR.cube_params(n=n)
    r_max = p.cube_x / 200.0
    rng = np.random.RandomState(8)
    pos = rng.uniform(0.0, p.cube_x, size=(n, 3))
    pos[:2000] = 0.37 * p.cube_x + rng.uniform(0.0, 10.0 * r_max, size=(2000, 3))
    pts = np.concatenate([pos, rng.normal(size=(n, 3)) * 300.0], axis=1)
    eng, g, state, ref = _crafted(pts, _cube_grid(r_max, 32, n=(2, 2, 2)))
    lo, hi, cells, edge = PA.search_box(g)
    assert cells == [128, 128, 128] and edge[0] > 1.5 * r_max
    tot = ref.check(eng)
    assert tot[:, 0].sum() == n and tot[:, 1:33].sum() > 4 * 2000 and (ref.n_outside, ref.n_unfiled) == (0, 0)
    eng.close()


# ---- 3. the pore: an axisymmetric grid ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [False, True])
def test_axisymmetric_grid_in_the_pore(wide):
    """2 (r) x 4 (z) regions at N = 4,096 with the default r_max = 32 d, and with r_max = 100 nm: larger than a region's radial
    width of 75 nm, so many pairs join two regions."""
    from argon_monte_carlo_amd.sim import Simulation
    sim = Simulation("pore", n=4096)
    p = sim.params
    sim.set_state(*IC.pore_ic(p, sim.consts, 21))
    r_max = 1.0e-7 if wide else 32.0 * float(p.collision_range)
    sim.enable_pairs(PA.make_grid("axisymmetric", (2, 4), (0.0, 0.0), (p.R_oa, p.H), r_max, hist_bins=16))
    assert (r_max > 0.5 * p.R_oa) == wide
    ref = Totals(sim.engine.pair_grid)
    sim.pairs_sample()
    ref.add_state(sim.engine.download())
    sim.timestep()
    sim.pairs_sample()
    ref.add_state(sim.engine.download())
    tot = ref.check(sim.engine)
    assert int(tot[:, 0].sum()) + ref.n_outside == 2 * 4096 and ref.n_unfiled == 0
    assert tot[:, 1:17].sum() > (100_000 if wide else 100)
    d = sim.pairs()
    assert d["g"].shape == (8, 16) and d["n_samples"] == 2 and np.isfinite(d["g"][d["centres"] > 0]).all()
    sim.close()


# ---- 4. deferred sweep results ---------------------------------------------------------------------------------------------------
def _dense_cube(n=3000, seed=10):
    """a dense cube (sixteen times the cross section: some forty collisions in every step), the binned detector"""
    from argon_monte_carlo_amd.sim import Simulation
    p, c = PR.cube_params_for_n(n, sigma=3.6e-19 * 16.0)
    p.detect_mode = 1
    sim = Simulation("cube", params=p, consts=c)
    sim.set_state(*IC.cube_ic(p, c, seed))
    return sim


def _small_grid(p, n=(1, 1, 1), ranges=8.0, hist_bins=16):
    return PA.make_grid("cartesian", n, (0, 0, 0), (p.cube_x, p.cube_y, p.cube_z), ranges * float(p.collision_range), hist_bins=hist_bins)


def test_sample_reads_through_the_deferred_results_of_the_last_sweep():
    """Straight after a timestep() whose collisions are still pending in the slot arrays, and again after the next step."""
    sim = _dense_cube()
    sim.enable_pairs(_small_grid(sim.params, (2, 1, 2)))
    ref = Totals(sim.engine.pair_grid)
    for _ in range(2):
        st = sim.timestep()
        assert st["n_pp"] >= 1                  # the sweep moved particles: their final state is in the slot arrays
        sim.pairs_sample()
        ref.add_state(sim.engine.download())
    tot = ref.check(sim.engine)
    d = sim.pairs()
    assert tot[:, 0].sum() + ref.n_outside == 6000 and tot[:, 1:17].sum() > 1000      # (a few particles have left the cube)
    # d = 2 columns of d / 2: the overlap count is exact here, and the scheme does leave pairs closer than d
    assert d["r_edges"][2] == float(sim.params.collision_range) and np.isfinite(d["overlap_per_centre"]).all()
    sim.close()


# ---- 5. launch geometry --------------------------------------------------------------------------------------------------------------
_GEOMETRY = {}


@pytest.mark.parametrize("blocks", [None, "1", "3"])
def test_totals_do_not_depend_on_the_number_of_workgroups(blocks, monkeypatch):
    if blocks is not None:
        monkeypatch.setenv("AMC_PAIR_BLOCKS", blocks)
    sim = _dense_cube(n=5000, seed=2)
    sim.enable_pairs(_small_grid(sim.params, (2, 2, 1), 4.0, 8), every=2)     # twelve cells per axis: the waves of 108 workgroups have a cell
    assert PA.search_box(sim.engine.pair_grid)[2] == [12, 12, 12]
    sim.run(4)
    got = sim.engine.pair_read()
    if "ref" not in _GEOMETRY:
        ref = Totals(sim.engine.pair_grid)
        one = _dense_cube(n=5000, seed=2)
        for s in range(4):
            one.timestep()
            if s % 2 == 1:
                ref.add_state(one.engine.download())
        one.close()
        _GEOMETRY["ref"] = ref.read()
    want = _GEOMETRY["ref"]
    assert got[1:] == want[1:] and got[1] == 2 and np.array_equal(got[0], want[0]), np.argwhere(got[0] != want[0])[:5]
    sim.close()


# ---- 6. the life cycle -----------------------------------------------------------------------------------------------------------
def test_cadence_with_step_offset_reset_and_load():
    sim = _dense_cube()
    g = _small_grid(sim.params)
    sim.engine.pair_config(PA.copy_grid(g, every=3, step_offset=1))        # after the steps s with (s + 1) % 3 == 0: 2, 5, 8
    sim.run(10)
    end = sim.engine.download()
    ref = Totals(g)
    one = _dense_cube()
    for s in range(1, 11):
        one.timestep()
        if (s + 1) % 3 == 0:
            ref.add_state(one.engine.download())
    last = one.engine.download()
    one.close()
    for k in KEYS:
        assert np.array_equal(end[k], last[k]), k
    tot = ref.check(sim.engine)
    assert ref.n_samples == 3 and tot[0, 0] + ref.n_outside == 9000
    # load: the inverse of read; a sample adds exactly to what was loaded
    big = (1 << 62) - 3
    loaded = np.arange(tot.size, dtype=np.int64).reshape(tot.shape) + big
    sim.engine.pair_load(loaded, 7, 5, 2)
    got = sim.engine.pair_read()
    assert got[1:] == (7, 5, 2) and np.array_equal(got[0], loaded)
    sim.pairs_sample()
    one_more = Totals(g)
    one_more.add_state(sim.engine.download())
    got = sim.engine.pair_read()
    assert got[1:] == (8, 5, 2) and np.array_equal(got[0], loaded + one_more.sums)
    with pytest.raises(ValueError):
        sim.engine.pair_load(loaded[:, :-1], 0, 0, 0)
    sim.pairs_reset()
    got = sim.engine.pair_read()
    assert got[1:] == (0, 0, 0) and not got[0].any()
    sim.close()


def test_checkpoint_saved_mid_run_resumes_to_the_uninterrupted_totals(tmp_path):
    ref = _dense_cube()
    ref.enable_pairs(every=3)
    ref.run(7)
    ref.run(8)
    want = ref.engine.pair_read()
    ref.close()
    a = _dense_cube()
    a.enable_pairs(every=3)
    a.run(7)
    ck = str(tmp_path / "ck.npz")
    a.save_checkpoint(ck)
    a.write_pairs(str(tmp_path / "pairs.npz"))
    a.close()
    zc = np.load(ck)
    assert zc["pair_grid"].shape == (14,) and zc["pair_totals"].shape == (1, 129) and zc["pair_counters"].tolist() == [2, 0, 0]
    z = np.load(str(tmp_path / "pairs.npz"))
    assert z["g"].shape == z["pairs"].shape == z["approach_fraction"].shape == (1, 64) and z["r_edges"].shape == (65,) and int(z["n_samples"]) == 2
    b = _dense_cube(seed=99)                # another state: the checkpoint brings its own
    b.load_checkpoint(ck)                   # restores the grid, the totals and the cadence (steps 9, 12, 15 still to come)
    b.run(8)
    got = b.engine.pair_read()
    assert got[1:] == want[1:] and got[1] == 5 and np.array_equal(got[0], want[0])
    b.close()
    c = _dense_cube()                       # a checkpoint without the sampler: it is off in the resumed run
    c.run(1)
    c.save_checkpoint(str(tmp_path / "plain.npz"))
    c.enable_pairs(every=1)
    c.load_checkpoint(str(tmp_path / "plain.npz"))
    assert c.engine.pair_grid is None
    c.close()


def test_state_errors_invalid_grids_and_reset_outputs():
    from argon_monte_carlo_amd._lib import ArgonMCError
    sim = _dense_cube(n=1000)
    lib, ctx = sim.engine.lib, sim.engine._ctx
    for call in (lib.amc_pair_sample, lib.amc_pair_reset):
        assert call(ctx) == -6
    assert lib.amc_pair_read(ctx, None, None, None, None) == -6
    one = np.zeros(1, dtype=np.int64)
    assert lib.amc_pair_load(ctx, one.ctypes.data_as(lib.amc_pair_load.argtypes[1]), 0, 0, 0) == -6
    with pytest.raises(ArgonMCError) as e:
        sim.engine.pair_read()
    assert e.value.code == -6
    sim.enable_pairs(every=1)
    sim.run(2)
    assert sim.engine.pair_read()[1] == 2
    sim.engine.reset_outputs()              # leaves the sampler alone
    tot, ns, no, nu = sim.engine.pair_read()
    assert ns == 2 and tot[0, 0] + no + nu == 2000
    sim.disable_pairs()                     # config(NULL): the state error is back
    with pytest.raises(ArgonMCError) as e:
        sim.pairs_sample()
    assert e.value.code == -6 and sim.engine.pair_grid is None and lib.amc_pair_reset(ctx) == -6
    for field, value in (("n1", 48), ("hist_bins", 257), ("hist_bins", 0), ("r_max", 0.0), ("r_max", -1.0), ("r_max", math.inf), ("r_max", math.nan)):
        g = PA.default_grid(sim.params)     # one region x 129 columns
        setattr(g, field, value)            # past the Python helper (n1 = 48: 6,192 columns): the library refuses it too
        with pytest.raises(ArgonMCError) as e:
            sim.engine.pair_config(g)
        assert e.value.code == -1, (field, value)
    g = PA.default_grid(sim.params)
    g.n1 = 47                               # 6,063 columns fit
    sim.engine.pair_config(g)
    sim.pairs_sample()
    assert sim.engine.pair_read()[1] == 1
    sim.close()


def test_sampling_leaves_step_statistics_and_state_unchanged():
    out = []
    for on in (False, True):
        sim = _dense_cube()
        if on:
            sim.enable_pairs(every=2)
        stats = [sim.run(10)]
        for _ in range(10):
            stats.append(sim.timestep())
        st = sim.engine.download()
        counts, npaths = sim.engine.histograms()
        out.append((st, stats, counts, npaths))
        if on:
            assert sim.engine.pair_read()[1] == 10
        sim.close()
    (a, sa, ca, na), (b, sb, cb, nb) = out
    for k in KEYS:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert sa == sb and na == nb and np.array_equal(ca, cb)


# ---- 7. the energised pore's host-free run ------------------------------------------------------------------------------------------
def _temp_sim(every):
    sim = make_temp_sim(True, n=6_000)
    p = sim.params
    sim.enable_pairs(PA.make_grid("axisymmetric", (1, 4), (0.0, 0.0), (p.R_oa, p.H), 32.0 * float(p.collision_range), hist_bins=8), every=every)
    return sim


def test_device_rng_run_samples_like_three_manual_samples():
    run = _temp_sim(2)
    run.run(6)
    got = run.engine.pair_read()
    end = run.engine.download()
    run.close()
    one = _temp_sim(0)
    ref = Totals(one.engine.pair_grid)
    for s in range(1, 7):
        one.timestep()
        if s % 2 == 0:
            one.pairs_sample()
            ref.add_state(one.engine.download())
    manual = one.engine.pair_read()
    last = one.engine.download()
    one.close()
    assert got[1] == manual[1] == 3 and got[1:] == manual[1:] and np.array_equal(got[0], manual[0])
    assert np.array_equal(got[0], ref.sums) and got[1:] == ref.read()[1:] and got[0][:, 1:9].sum() > 0
    for k in KEYS:
        assert np.array_equal(end[k], last[k]), k


# ---- 8. three ranks with uneven ranges in one process ---------------------------------------------------------------------------
class _ThreadComm:
    """The one collective ShardedSimulation.pairs() needs, among threads of one process: every rank's list summed element-wise."""

    def __init__(self, world):
        import threading
        self.world, self.shortcut, self.parts = world, False, {}
        self.barrier = threading.Barrier(world)

    def view(self, rank):
        comm = self

        class View:
            shortcut = False

            def allreduce_sum_ints(self, values):
                comm.parts[rank] = [int(v) for v in values]
                comm.barrier.wait()
                out = [sum(col) for col in zip(*(comm.parts[r] for r in range(comm.world)))]
                comm.barrier.wait()         # (nobody overwrites its part before everybody has summed)
                return out
        return View()


def _sharded_pairs(p, engs):
    """ShardedSimulation.pairs() of every rank over the given engines, the ranks as threads: [dict per rank]"""
    import threading
    from argon_monte_carlo_amd.dist import ShardedSimulation
    comm = _ThreadComm(len(engs))
    sims = [ShardedSimulation(p, r, len(engs), engine=e, comm=comm.view(r)) for r, e in enumerate(engs)]
    out, errors = [None] * len(engs), []

    def work(r):
        try:
            out[r] = sims[r].pairs()
        except BaseException as e:          # noqa: BLE001  (reported by the test's thread)
            errors.append((r, e))
            comm.barrier.abort()
    threads = [threading.Thread(target=work, args=(r,)) for r in range(len(engs))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    return out


def test_three_ranks_sum_to_the_single_context():
    """Every rank holds the whole system and counts the centres of its own index range against everybody: the totals and n_outside
    add up to the single context's, n_unfiled is the whole system's on every rank."""
    from argon_monte_carlo_amd.dist import LocalRanks, shard_range
    from argon_monte_carlo_amd.engine import Engine, ShardEngine
    n, steps, every = 3001, 4, 2
    p, c = PR.cube_params_for_n(n, sigma=3.6e-19 * 16.0)
    p.detect_mode = 1
    init = IC.cube_ic(p, c, 10)
    # a grid over the lower half in x: the upper half is outside, and beyond r_max from it unfiled
    g = PA.make_grid("cartesian", (2, 1, 1), (0, 0, 0), (0.5 * p.cube_x, p.cube_y, p.cube_z), 8.0 * float(p.collision_range), hist_bins=16, every=every)
    eng = Engine(p)
    eng.upload(*init)
    eng.pair_config(g)
    ref = Totals(g)
    for s in range(1, steps + 1):
        assert eng.timestep(c["dt"])["n_pp"] >= 1
        if s % every == 0:
            ref.add_state(eng.download())
    want = ref.check(eng)
    eng.close()
    assert ref.n_outside > 0 and ref.n_unfiled > 0 and want[:, 1:17].sum() > 100
    ranges = [shard_range(n, r, 3) for r in range(3)]
    assert [hi - lo for lo, hi in ranges] == [1001, 1000, 1000]
    stream = torch.cuda.current_stream().cuda_stream
    engs = [ShardEngine(p, lo, hi) for lo, hi in ranges]
    for e in engs:
        e.set_stream(stream)
        e.upload(*init)
        e.pair_config(g)
    job = LocalRanks(engs)
    for _ in range(steps):
        job.step(c["dt"])
    reads = [e.pair_read() for e in engs]
    derived = _sharded_pairs(p, engs)
    for e in engs:
        e.close()
    # ShardedSimulation.pairs() on every rank: the summed totals and n_outside, the sample count, and n_unfiled as the rank's own
    # value (the whole system's: a sum over the ranks would be three times it)
    for d in derived:
        assert np.array_equal(d["totals"], want) and d["totals"].dtype == np.int64
        assert (d["n_samples"], d["n_outside"], d["n_unfiled"]) == (ref.n_samples, ref.n_outside, ref.n_unfiled)
        assert np.array_equal(d["centres"], want[:, 0]) and d["g"].shape == (2, 16)
    assert np.array_equal(sum(r[0] for r in reads), want)
    assert all(r[1] == ref.n_samples for r in reads) and sum(r[2] for r in reads) == ref.n_outside
    assert all(r[3] == ref.n_unfiled for r in reads)        # the whole system's, on every rank: a sum would count it three times
    assert all(0 < r[0][:, 0].sum() < want[:, 0].sum() for r in reads)


# ---- 9. the pore geometries: one rank over the whole range samples, an index-range shard is refused -----------------------------
def _dense_pore(n=8000):
    """a pore with 64 times the cross section: a few collisions per step at N = 8,000"""
    p, c = PR.pore_params(n=n, sigma=3.6e-19 * 64.0)
    p.detect_mode = 1
    return p, c, IC.pore_ic(p, c, 11)


def test_pore_one_rank_over_the_whole_range_through_the_sharded_step():
    """amc_mg_finish's pore path: the owner's bounds pass consumes the deferred results before the hook — the owner of everybody
    then holds everybody's final state."""
    from argon_monte_carlo_amd.dist import LocalRanks
    from argon_monte_carlo_amd.engine import ShardEngine
    p, c, init = _dense_pore()
    g = PA.make_grid("axisymmetric", (1, 4), (0.0, 0.0), (p.R_oa, p.H), 8.0 * float(p.collision_range), hist_bins=16, every=2)
    eng = ShardEngine(p, 0, int(p.n))
    eng.upload(*init)
    eng.pair_config(g)
    job = LocalRanks([eng])
    ref = Totals(g)
    n_pp = 0
    for s in range(1, 7):
        n_pp += job.step(c["dt"], want_stats=True)[0]["n_pp"]
        if s % 2 == 0:
            ref.add_state(eng.download())
    print("p-p collisions in six steps:", n_pp)
    assert n_pp >= 1
    tot = ref.check(eng)
    assert ref.n_samples == 3 and tot[:, 1:17].sum() > 0
    eng.close()


def test_pore_shard_is_refused_with_a_clear_error():
    """On an index-range shard of a pore geometry the other shards' final state of a step is not resident (the owner's bounds pass
    has consumed the deferred results): configuring, sampling and the cadence hook fail with AMC_ERR_STATE."""
    from argon_monte_carlo_amd._lib import ArgonMCError
    from argon_monte_carlo_amd.dist import LocalRanks, shard_range
    from argon_monte_carlo_amd.engine import ShardEngine
    p, c, init = _dense_pore(3001)
    g = PA.make_grid("axisymmetric", (1, 4), (0.0, 0.0), (p.R_oa, p.H), 8.0 * float(p.collision_range), hist_bins=16, every=1)
    engs = [ShardEngine(p, *shard_range(3001, r, 3)) for r in range(3)]
    stream = torch.cuda.current_stream().cuda_stream
    for e in engs:
        e.set_stream(stream)
        e.upload(*init)
        with pytest.raises(ArgonMCError, match="index-range shard") as err:
            e.pair_config(g)
        assert err.value.code == -6 and e.pair_grid is None
    # a grid configured while the context still held the whole range: the sample and the step's hook refuse
    whole = ShardEngine(p, 0, 3001)
    whole.upload(*init)
    whole.pair_config(g)
    whole._ck(whole.lib.amc_set_shard(whole._ctx, 0, 1500))
    with pytest.raises(ArgonMCError, match="index-range shard") as err:
        whole.pair_sample()
    assert err.value.code == -6
    job = LocalRanks([whole])
    with pytest.raises(ArgonMCError, match="index-range shard"):
        job.step(c["dt"])
    assert whole.pair_read()[1] == 0
    whole.close()
    for e in engs:
        e.close()


# ---- 12. the reduce at its shapes -------------------------------------------------------------------------------------------------
_REDUCE_REF = {}


def _reduce_case(regions):
    """(params, grid of ``regions`` regions over the lower half of the pore's box, state, the mirror's sample), computed once"""
    from tests.sampler_states import ODD_N, drifting_states
    if regions not in _REDUCE_REF:
        p, (st,) = drifting_states(ODD_N, 1, seed=29)
        g = PA.make_grid("cartesian", (regions, 1, 1), (-p.R_oa, -p.R_oa, 0.0), (p.R_oa, p.R_oa, 0.5 * p.H), 2.0e-8,
                         hist_bins={21: 1, 13: 2}[regions])
        _REDUCE_REF[regions] = (p, g, st) + REF.sample(g, *st)
    return _REDUCE_REF[regions]


@pytest.mark.parametrize("blocks", ["1", "17", "33"])
@pytest.mark.parametrize("regions", [21, 13])
def test_reduce_shapes_equal_reference(regions, blocks, monkeypatch):
    """21 regions of H = 1: W = 21 * 3 = 63 totals columns, the counters' thread is lane 63 of the reduce's only workgroup; 13
    regions of H = 2: W = 13 * 5 = 65, the counters' thread is lane 1 of a second one.  1, 17 and 33 slab rows: below, one above and
    two above a multiple of the reduce's sixteen waves.  The counters' thread folds the side words in and leaves them and the cell
    cursor at zero: a sample that found them otherwise would count twice, or no cell at all."""
    from argon_monte_carlo_amd.engine import Engine
    p, g, st, sums, outside, unfiled = _reduce_case(regions)
    assert sums.size == {21: 63, 13: 65}[regions] and outside > 0 and unfiled > 0 and (sums[:, 0] > 0).all() and (sums[:, 1:].sum(axis=0) > 0).all()
    monkeypatch.setenv("AMC_PAIR_BLOCKS", blocks)
    eng = Engine(p)
    eng.upload(*st)
    eng.pair_config(g)
    for k in (1, 2, 3):                 # (the later samples add onto non-zero totals)
        eng.pair_sample()
        tot, ns, no, nu = eng.pair_read()
        assert (ns, no, nu) == (k, k * outside, k * unfiled)
        assert np.array_equal(tot, k * sums), np.argwhere(tot != k * sums)[:5]
    eng.close()
