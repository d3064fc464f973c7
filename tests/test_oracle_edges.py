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
