"""The oracle against the REFERENCE ITSELF on the crafted edge inputs (tests/golden/func_edge.npz, made by
`oracle/gen_golden.py --only edge` from tests/edge_states.py): planes and cylinders hit exactly, tangential and rootless
side-wall solves, the bounds thresholds, pairs at the collision distance.  Bar: `pow` bit-for-bit; `mul` the same events,
outputs within the ulps test_mul_mode_differs_only_in_ulps allows.  Without this pin, GPU == oracle at an edge would
prove nothing about the reference.

Also (CPU only): every crafted state stays finite through the oracle and contains every case it claims."""
import os

import numpy as np
import pytest

from argon_monte_carlo_amd import params as PR
from argon_monte_carlo_amd._abi import AMC_ERR_FP
from oracle import gen_golden as GG
from oracle import oracle as O
from tests import edge_states as E

STATE_KEYS = ["x_vals", "y_vals", "z_vals", "x_velocities", "y_velocities", "z_velocities", "dist_since_collision",
              "dist_x_since_collision", "dist_y_since_collision", "dist_z_since_collision", "full_path_traveled"]
FIELDS = ["cont", "cx", "cy", "cz", "flag", "x", "y", "z", "vx", "vy", "vz"]


@pytest.fixture(scope="module")
def G(golden_dir):
    return np.load(os.path.join(golden_dir, "func_edge.npz"))


def test_fixture_inputs_are_the_builders(G):
    """the fixture still belongs to tests/edge_states.py (rerun `gen_golden.py --only edge` after changing a builder)"""
    for k, v in GG.edge_inputs().items():
        assert np.array_equal(np.asarray(v), G[k]), k


def _wall_oracle(G, mode, sl=slice(None)):
    n = len(G["wall_in_x_vals"][sl])
    p = PR.pore_params(n=n)[0]
    o = O.Oracle(p, mode=mode)
    o.upload(*[G[f"wall_in_{k}"][sl] for k in STATE_KEYS[:10]], flag=G["wall_in_full_path_traveled"][sl])
    return o


def _paths(o):
    r = o.paths()
    return np.stack([r["total"], r["px"], r["py"], r["pz"]], axis=1)


@pytest.mark.parametrize("q", range(len(GG.EDGE_PLANES)))
def test_hit_vertical_wall_on_edges(G, q):
    pre = f"vedge{q}"
    hits = G[f"{pre}_hits"]
    assert hits.sum() >= 10
    # coverage: particles exactly on the plane (t == 0)
    zp = float(G[f"{pre}_plane"])
    z = G["wall_in_z_vals"][hits]
    assert (z == zp).sum() >= 2
    res = {}
    for mode in ("pow", "mul"):
        o = _wall_oracle(G, mode)
        nc = o.vertical_wall(hits, zp)
        assert nc == int(G[f"{pre}_ncoll"])
        res[mode] = (o.state(), _paths(o))
    st, paths = res["pow"]
    for k, f in zip(STATE_KEYS[:10], O.STATE_FIELDS):
        assert np.array_equal(st[f], G[f"{pre}_out_{k}"]), (pre, k)
    assert np.array_equal(st["flag"].astype(bool), G[f"{pre}_out_full_path_traveled"])
    assert np.array_equal(paths, G[f"{pre}_paths"])
    sm, pm = res["mul"]
    for f in O.STATE_FIELDS:
        np.testing.assert_allclose(sm[f], st[f], rtol=1e-9, atol=0)
    np.testing.assert_allclose(pm, paths, rtol=1e-9, atol=0)


@pytest.mark.parametrize("mode", ["pow", "mul"])
def test_hit_cylinder_side_wall_on_edges(G, mode):
    idx, Rcs, outcome = G["sedge_idx"], G["sedge_Rc"], G["sedge_outcome"]
    assert outcome.sum() >= 6 and (outcome == 0).sum() >= 20           # both outcomes are exercised
    for m, (i, Rc) in enumerate(zip(idx, Rcs)):
        o = _wall_oracle(G, mode, slice(int(i), int(i) + 1))
        rc, nc, nerr = o.side_wall(np.array([1], dtype=np.uint8), float(Rc))
        if outcome[m]:
            assert rc == AMC_ERR_FP, (m, i)       # the reference's call raised: the oracle reports a failed solve
            continue
        assert rc == 0 and nc == 1, (m, i, rc)
        st = o.state()
        for k, f in zip(STATE_KEYS[:10], O.STATE_FIELDS):
            exp = G[f"sedge_out_{k}"][m]
            if mode == "pow":
                assert st[f][0] == exp, (m, i, k, st[f][0], exp)
            else:
                np.testing.assert_allclose(st[f][0], exp, rtol=1e-9, atol=0, err_msg=f"{m} {k}")
        got = _paths(o)
        exp = G["sedge_paths"][m]
        if np.isnan(exp).all():
            assert len(got) == 0
        elif mode == "pow":
            assert np.array_equal(got[0], exp), m
        else:
            np.testing.assert_allclose(got[0], exp, rtol=1e-9, atol=0)


def test_side_wall_edges_tolerated_with_reserved1(G):
    """reserved1 bit0: the same rootless solves are counted and the particle is left alone"""
    idx, Rcs, outcome = G["sedge_idx"], G["sedge_Rc"], G["sedge_outcome"]
    for m in np.flatnonzero(outcome):
        i = int(idx[m])
        o = _wall_oracle(G, "pow", slice(i, i + 1))
        o.p.reserved1 = 1
        before = o.state()
        rc, nc, nerr = o.side_wall(np.array([1], dtype=np.uint8), float(Rcs[m]))
        assert rc == 0 and nerr == 1
        after = o.state()
        for f in O.STATE_FIELDS:
            assert np.array_equal(before[f], after[f])


def test_num_out_of_bounds_on_thresholds(G):
    n = len(G["bedge_in_x"])
    p = PR.pore_params(n=n)[0]
    z = np.zeros(n)
    for mode in ("pow", "mul"):
        o = O.Oracle(p, mode=mode)
        o.upload(G["bedge_in_x"], G["bedge_in_y"], G["bedge_in_z"], z, z, z)
        cnt = o.bounds(False)
        assert cnt == int(G["bedge_count"]) and 0 < cnt < n
        st = o.state()
        for f in ("x", "y", "z"):
            assert np.array_equal(st[f], G[f"bedge_out_{f}"]), (mode, f)


def _run_pair(G, k, mode):
    p = PR.cell_params(n=2)[0]
    return O.pair_cell(p, *[G[f"pedge_in_{f}"][k] for f in FIELDS], mode=mode)


def test_pairs_at_the_collision_distance(G):
    n = G["pedge_in_x"].shape[0]
    hit = 0
    for k in range(n):
        a, pa, nca, rca = _run_pair(G, k, "pow")
        b, pb, ncb, rcb = _run_pair(G, k, "mul")
        assert rca == rcb == 0
        assert nca == ncb == G["pedge_ncoll"][k], k
        for f in FIELDS:
            assert np.array_equal(a[f].astype(np.float64), G[f"pedge_out_{f}"][k]), (k, f)
            np.testing.assert_allclose(b[f].astype(np.float64), a[f].astype(np.float64), rtol=1e-9, atol=0)
        for q in range(len(pa)):
            assert np.array_equal(pa[q], G["pedge_paths"][k, q])
            np.testing.assert_allclose(pb[q], pa[q], rtol=1e-9, atol=0)
        hit += nca
    assert 0 < hit < n                                                 # both sides of the collision distance


# ---------------------------------------------------------------------------------------------------------- energised walls
# tests/golden/func_temp_edge.npz (`oracle/gen_golden.py --only temp_edge`): Temperature_Pore_MC.py itself for one step on
# tests/edge_states.temp_walls(reference_safe=True) — its seven masks (inline in its main loop: no function-level fixture
# reaches them), the state after the cases and after the step, its error count, paths and sums.
@pytest.fixture(scope="module")
def GT(golden_dir):
    return np.load(os.path.join(golden_dir, "func_temp_edge.npz"))


def _ref_masks(GT):
    n = len(GT["s-001_x_vals"])
    return {k: np.unpackbits(GT["c_" + name])[:n].astype(bool) for k, name in GG.TEMP_MASKS.items()}


def test_temp_fixture_inputs_are_the_builders(GT):
    """the fixture still belongs to tests/edge_states.py (rerun `gen_golden.py --only temp_edge` after changing temp_walls)"""
    for k, v in GG.temp_edge_inputs().items():
        assert np.array_equal(np.asarray(v), GT["s-001_" + k]), k


def test_oracle_reproduces_the_reference_on_the_energised_edges(GT):
    """The oracle (`pow`, the reference's RNG states, its own host loop) on the crafted energised state: the seven masks,
    the state after the cases and after the step, the paths (a multiset: the sweep's workers append in scheduling order),
    total_errs and the three sums, bit for bit."""
    import random
    from oracle import temp_host as TH
    from tests.test_oracle_steps import restore_rngs
    n = int(GT["meta_K"])
    p, c = PR.pore_params(n=n, energised=True)
    assert p.collision_range == float(GT["collision_range"]) and c["dt"] == float(GT["dt"])
    restore_rngs(GT)
    o = O.Oracle(p, mode="pow")
    o.upload(*[GT[f"s-001_{k}"] for k in STATE_KEYS[:10]], flag=GT["s-001_full_path_traveled"])

    class Recording:
        masks = {}

        def wall_hits(self, case):
            r = o.wall_hits(case)
            self.masks[case] = np.isin(np.arange(n), r[0])
            return r

        def wall_apply(self, *a):
            return o.wall_apply(*a)

    o._temp_wall_count = o._temp_errs = 0
    o.drift(c["dt"], True)
    o._temp_errs += o.temp_specular()
    mom, cold, hot, *_ = TH.run_cases(Recording(), TH.Directions(np.random, random), TH.Energies(c))
    ref = _ref_masks(GT)
    for k in ref:
        assert np.array_equal(Recording.masks[k], ref[k]), (k, np.flatnonzero(Recording.masks[k] != ref[k]))

    def same_state(tag):
        st = o.state()
        for k, f in zip(STATE_KEYS[:10], O.STATE_FIELDS):
            assert np.array_equal(st[f], GT[f"{tag}_{k}"]), (tag, k, np.flatnonzero(st[f] != GT[f"{tag}_{k}"])[:5])
        assert np.array_equal(st["flag"].astype(bool), GT[f"{tag}_full_path_traveled"]), tag

    def rows(r):
        a = np.stack([r["total"], r["px"], r["py"], r["pz"]], axis=1)
        return a[np.lexsort(a.T[::-1])]

    same_state("c")
    cp = GT["c_paths"]
    assert np.array_equal(rows(o.paths()), cp[np.lexsort(cp.T[::-1])])
    assert o._temp_errs == int(GT["c_total_errs"]) == int(GT["total_errs"])
    for got, key in ((mom, "momentum_z_change_in_step"), (cold, "energy_change_cold_in_step"), (hot, "energy_change_hot_in_step")):
        assert float(got) == float(GT["c_" + key]) != 0.0, key
    o.bounds(True)
    rc, npp, _ = o.sweep()
    o.bounds(True)
    assert rc == 0 and npp + o._temp_wall_count == int(GT["per_step"][0, 1]) == int(GT["total_cols"])
    same_state("s0000")
    assert np.array_equal(rows(o.paths()), GT["completed_rows"])


# Temp:708-751, one row per comparison: (case id, left side, operator, threshold, where a particle EXACTLY on the threshold is)
TEMP_COMPARISONS = [
    (3, "pz", ">=", "t_z3_cold", "in"), (3, "z", "<", "t_z3_cold", "out"), (3, "r2", ">", "R_p_sq", "out"),
    (4, "pz", "<=", "t_z3_hot", "in"), (4, "z", ">", "t_z3_hot", "out"), (4, "r2", ">", "R_p_sq", "out"),
    (5, "pz", "<", "t_zgap_hi", "out"), (5, "pz", ">", "t_zgap_lo", "out"), (5, "r02", "<=", "R_g_c_sq", "in"),
    (5, "r2", ">", "R_g_c_sq", "out"),
    (6, "r02", ">=", "R_p_c_sq", "in"), (6, "z", "<", "t_zgap_lo", "out"), (6, "pz", "<=", "t_zgap_hi", "in"),
    (6, "pz", ">=", "t_zgap_lo", "in"),
    (7, "r02", ">=", "R_p_c_sq", "in"), (7, "z", ">", "t_zgap_hi", "out"), (7, "pz", "<=", "t_zgap_hi", "in"),
    (7, "pz", ">=", "t_zgap_lo", "in"),
    (8, "r02", "<=", "R_p_c_sq", "in"), (8, "r2", ">", "R_p_c_sq", "out"), (8, "z", "<=", "t_zgap_lo", "in"),
    (8, "z", ">=", "t_z3_hot", "in"),
    (9, "r02", "<=", "R_p_c_sq", "in"), (9, "r2", ">", "R_p_c_sq", "out"), (9, "z", "<", "t_z3_cold", "out"),
    (9, "z", ">", "t_zgap_hi", "out"),
]


def test_the_reference_ran_the_energised_edges(GT):
    """On the FIXTURE: the reference itself hit every case, took the corner sequences (4 then 8, 5 then 6, 5 then 7, 6 then
    8 from a prior radius^2 == R_p_c_sq; 3 then 9 and 7 then 9 blocked), met a solve without a real root, and put the
    particle exactly on each threshold inside or outside the mask as the operator of Temp:708-751 says."""
    import operator
    s = E.temp_walls(reference_safe=True)
    masks = _ref_masks(GT)
    E.assert_temp_coverage(s, {k: np.flatnonzero(v) for k, v in masks.items()}, int(GT["total_errs"]))
    assert len(TEMP_COMPARISONS) == 26 and len(set(TEMP_COMPARISONS)) == 26
    # what a mask saw of a particle that no earlier case moved: the prior position as uploaded, the drift's own arithmetic
    dt, p = float(GT["dt"]), s.p
    x, y, z = s.x + dt * s.vx, s.y + dt * s.vy, s.z + dt * s.vz
    val = {"z": z, "pz": s.z, "r2": x ** 2 + y ** 2, "r02": s.x ** 2 + s.y ** 2}
    ops = {"<": operator.lt, "<=": operator.le, ">": operator.gt, ">=": operator.ge}
    untouched = np.ones(s.n, dtype=bool)
    for case in range(3, 10):
        mine = [row for row in TEMP_COMPARISONS if row[0] == case]
        for row in mine:
            _, lhs, op, thr, side = row
            assert side == ("in" if "=" in op else "out"), row
            others = np.ones(s.n, dtype=bool)
            for _, l2, o2, t2, _ in mine:
                if (l2, o2, t2) != (lhs, op, thr):
                    others &= ops[o2](val[l2], getattr(p, t2))
            on = np.flatnonzero(untouched & others & (val[lhs] == getattr(p, thr)))
            assert len(on) >= 1, ("no particle exactly on", row)
            assert np.all(masks[case][on] == (side == "in")), (row, on, masks[case][on])
        untouched &= ~masks[case]


# ---------------------------------------------------------------------------------------------------------- the builders
def _through_oracle(s, steps, **prm):
    for k, v in prm.items():
        setattr(s.p, k, v)
    o = O.Oracle(s.p, mode="mul")
    a = s.arrays()
    o.upload(*a[:10], flag=a[10])
    for q in range(steps):
        rc, _ = o.timestep(s.dt)
        assert rc == 0, q
        st = o.state()
        for f in O.STATE_FIELDS:
            assert np.isfinite(st[f]).all(), (q, f)
    return o


@pytest.mark.parametrize("name", ["walls", "walls_fp", "cube", "cell_pore", "cell_cube", "grid_pore", "grid_cube", "hist"])
def test_edge_states_stay_finite_through_the_oracle(name):
    s, prm = {"walls": (E.pore_walls(), {}), "walls_fp": (E.pore_walls(True), dict(reserved1=1)),
              "cube": (E.cube_walls(), {}), "cell_pore": (E.cell_pairs("pore"), {}), "cell_cube": (E.cell_pairs("cube"), {}),
              "grid_pore": (E.grid_pairs("pore"), {}), "grid_cube": (E.grid_pairs("cube"), {}),
              "hist": (E.hist_state(0.0, 1e-6, 200), {})}[name]
    assert all(len(v) > 0 for v in s.cases.values())
    o = _through_oracle(s, 4, **prm)
    r = o.paths()
    for k in ("total", "px", "py", "pz"):
        assert np.isfinite(r[k]).all() or name == "hist"


def test_landed_positions_sit_on_their_edges():
    """the drift's own arithmetic puts landed coordinates exactly on the edge values"""
    s = E.pore_walls()
    p = s.p
    for name, zp in (("zero", 0.0), ("H", p.H), ("z_cold", p.z_cold), ("h_oa", p.h_oa), ("z_gap_bottom", p.z_gap_bottom),
                     ("z_gap_top", p.z_gap_top)):
        idx = s.cases[f"cur_z_{name}"]
        z1 = s.z[idx] + s.dt * s.vz[idx]
        assert (z1 == zp).sum() >= 2, name
    c = E.cell_pairs("pore")
    x1 = c.x + c.dt * c.vx
    faces = np.arange(-7, 8) * c.p.dx
    assert np.isin(x1, faces).sum() >= 8 and np.isin(x1, faces - c.p.overlap_x).sum() >= 8


def test_histogram_values_exercise_the_fix_up():
    """np.histogram's uniform-bin path takes a first guess and fixes it against the edges lo + k*step: among the chosen
    values (tests/edge_states.hist_values over HIST_RANGES) the kernel's first guess is moved down for some and up for
    some, the up move also at exact edges (v >= e1)"""
    down = up = up_on_edge = on_edge = 0
    for lo, hi, nb in E.HIST_RANGES:
        v = np.abs(E.hist_values(lo, hi, nb))
        edges = np.linspace(lo, hi, nb + 1)
        on_edge += int(np.isin(v, edges).sum())
        v = v[np.isfinite(v) & (v >= lo) & (v <= hi)]
        g, t = E.hist_guess(v, lo, hi, nb), E.hist_true_bin(v, lo, hi, nb)
        ref = np.histogram(v, bins=nb, range=(lo, hi))[0]
        assert np.array_equal(np.bincount(t, minlength=nb), ref)        # the helper is np.histogram's binning
        down += int((t < g).sum())
        up += int((t > g).sum())
        up_on_edge += int(((t > g) & np.isin(v, edges)).sum())
    assert down >= 10 and up >= 10 and up_on_edge >= 10 and on_edge >= 400
