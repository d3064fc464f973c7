#!/usr/bin/env python3
"""Generate the golden vectors under tests/golden/ from the REFERENCE ITSELF (build container only).

    MPLBACKEND=Agg PYTHONDONTWRITEBYTECODE=1 python3 oracle/gen_golden.py [--only func|edge|clusters|resolve|temp_edge|cube|pore|temp|consts|cube_natural|pore_natural]

* function level: imports /root/reference/Open_Air_Pore_MC.py (its main loop is __main__-guarded) and calls
  pairwise_particles_in_cell / hit_vertical_wall / hit_cylinder_side_wall / num_out_of_bounds on seeded inputs
  (func) and on the crafted edge inputs of tests/edge_states.py (edge).
* step level: writes a PATCHED TEMPORARY COPY of a reference script into a scratch directory under /tmp
  (single-line substitutions of num_molecules / sigma / slice count / loop bound, plus calls to a dump hook after
  every step), runs it there as a script and collects the dumps.  Nothing of the reference's text is stored in
  the repository: the fixtures hold only inputs, outputs and the patch PARAMETERS.

The reference does not exist on the GPU box; the fixtures travel instead.
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(os.path.dirname(HERE), "tests", "golden")

STATE_KEYS = ["x_vals", "y_vals", "z_vals", "x_velocities", "y_velocities", "z_velocities", "dist_since_collision",
              "dist_x_since_collision", "dist_y_since_collision", "dist_z_since_collision", "full_path_traveled"]


# ------------------------------------------------------------------------------------------------ function level
def gen_func():
    os.environ.setdefault("MPLBACKEND", "Agg")
    sys.path.insert(0, REF)
    import multiprocessing
    import Open_Air_Pore_MC as P  # noqa

    rng = np.random.default_rng(20240917)
    cr = float(P.collision_range)
    out = {}

    # --- (i) single pairs -------------------------------------------------------------------------------
    npair = 1000
    fields = ["cont", "cx", "cy", "cz", "flag", "x", "y", "z", "vx", "vy", "vz"]
    pin = {k: np.zeros((npair, 2)) for k in fields}
    pout = {k: np.zeros((npair, 2)) for k in fields}
    paths = np.full((npair, 2, 4), np.nan)
    npaths = np.zeros(npair, dtype=np.int64)
    ncoll = np.zeros(npair, dtype=np.int64)
    for k in range(npair):
        ctr = Value = None
        counter = multiprocessing.Value('i', 0)
        P.init_globals(counter)
        base = rng.uniform(-1e-7, 1e-7, 3) + np.array([0, 0, 1.5e-6])
        sep = cr * rng.uniform(0.05, 1.3 if k % 5 == 0 else 0.999)
        u = rng.normal(size=3); u /= np.linalg.norm(u)
        pos = np.stack([base, base + sep * u])
        vel = rng.normal(size=(2, 3)) * 249.0
        if k % 3 == 0:  # make them approach head-on-ish
            vel[1] = vel[0] - u * abs(rng.normal()) * 300 + rng.normal(size=3) * 30
        cont = rng.uniform(0, 2e-7, (2, 4))
        cont[:, 0] = np.sqrt((cont[:, 1:] ** 2).sum(1)) * rng.uniform(1, 1.5)
        flag = rng.integers(0, 2, 2).astype(bool)
        args = [cont[:, 0].copy(), cont[:, 1].copy(), cont[:, 2].copy(), cont[:, 3].copy(), flag.copy(),
                pos[:, 0].copy(), pos[:, 1].copy(), pos[:, 2].copy(), vel[:, 0].copy(), vel[:, 1].copy(), vel[:, 2].copy()]
        for f, a in zip(fields, args):
            pin[f][k] = a
        lists = [[], [], [], []]
        res = P.pairwise_particles_in_cell(lists[0], lists[1], lists[2], lists[3], np.array([True, True]), *args)
        for f, a in zip(fields, res[1:]):
            pout[f][k] = a
        npaths[k] = len(lists[0])
        for q in range(len(lists[0])):
            paths[k, q] = [lists[0][q], lists[1][q], lists[2][q], lists[3][q]]
        ncoll[k] = counter.value
    for f in fields:
        out["pair_in_" + f] = pin[f]
        out["pair_out_" + f] = pout[f]
    out["pair_paths"] = paths
    out["pair_npaths"] = npaths
    out["pair_ncoll"] = ncoll

    # --- (ii) whole cells with chained collisions -----------------------------------------------------------
    ncells = 24
    cell_sizes = rng.integers(40, 301, ncells)
    cell_sizes[:4] = [2, 3, 5, 300]
    off = np.concatenate([[0], np.cumsum(cell_sizes)])
    tot = int(off[-1])
    cin = {k: np.zeros(tot) for k in fields}
    cout = {k: np.zeros(tot) for k in fields}
    cpaths = []
    cpath_off = [0]
    cncoll = np.zeros(ncells, dtype=np.int64)
    for c in range(ncells):
        n = int(cell_sizes[c])
        counter = multiprocessing.Value('i', 0)
        P.init_globals(counter)
        # pack n spheres into a box whose volume gives ~8-25% volume fraction => several overlaps + chains
        vf = rng.uniform(0.08, 0.25)
        side = (n * (4.0 / 3.0) * np.pi * (cr / 2) ** 3 / vf) ** (1.0 / 3.0)
        pos = rng.uniform(0, side, (n, 3)) + np.array([1e-8, -2e-8, 1.2e-6])
        vel = rng.normal(size=(n, 3)) * 249.0
        cont = rng.uniform(0, 2e-7, (n, 4))
        flag = rng.integers(0, 2, n).astype(bool)
        args = [cont[:, 0].copy(), cont[:, 1].copy(), cont[:, 2].copy(), cont[:, 3].copy(), flag.copy(),
                pos[:, 0].copy(), pos[:, 1].copy(), pos[:, 2].copy(), vel[:, 0].copy(), vel[:, 1].copy(), vel[:, 2].copy()]
        for f, a in zip(fields, args):
            cin[f][off[c]:off[c + 1]] = a
        lists = [[], [], [], []]
        res = P.pairwise_particles_in_cell(lists[0], lists[1], lists[2], lists[3], np.ones(n, dtype=bool), *args)
        for f, a in zip(fields, res[1:]):
            cout[f][off[c]:off[c + 1]] = a
        cpaths.extend(zip(*lists))
        cpath_off.append(len(cpaths))
        cncoll[c] = counter.value
    for f in fields:
        out["cell_in_" + f] = cin[f]
        out["cell_out_" + f] = cout[f]
    out["cell_off"] = off
    out["cell_paths"] = np.array(cpaths, dtype=np.float64).reshape(-1, 4)
    out["cell_path_off"] = np.array(cpath_off)
    out["cell_ncoll"] = cncoll

    # --- (iii) wall handlers --------------------------------------------------------------------------------
    def set_state(n):
        st = {}
        st["x_vals"] = rng.uniform(-1.6e-7, 1.6e-7, n)
        st["y_vals"] = rng.uniform(-1.6e-7, 1.6e-7, n)
        st["z_vals"] = rng.uniform(-2e-8, 3.22e-6, n)
        for k in ["x_velocities", "y_velocities", "z_velocities"]:
            st[k] = rng.normal(size=n) * 249.0
        for k in ["dist_since_collision", "dist_x_since_collision", "dist_y_since_collision", "dist_z_since_collision"]:
            st[k] = rng.uniform(0, 3e-7, n)
        st["full_path_traveled"] = rng.integers(0, 2, n).astype(bool)
        return st

    def load(st):
        for k, v in st.items():
            setattr(P, k, v.copy())

    def grab():
        return {k: getattr(P, k).copy() for k in STATE_KEYS}

    nw = 300
    # vertical walls at several planes
    vplanes = [0.0, float(P.total_height), float(P.total_height - P.open_air_height), float(P.open_air_height),
               float(P.open_air_height + P.hot_coating_height)]
    for q, zp in enumerate(vplanes):
        st = set_state(nw)
        hits = rng.random(nw) < 0.4
        load(st)
        counter = multiprocessing.Value('i', 0)
        P.num_collisions_per_step = counter
        lists = [[], [], [], []]
        P.hit_vertical_wall(hits, zp, *lists)
        res = grab()
        for k in STATE_KEYS:
            out[f"vwall{q}_in_{k}"] = st[k]
            out[f"vwall{q}_out_{k}"] = res[k]
        out[f"vwall{q}_hits"] = hits
        out[f"vwall{q}_plane"] = np.float64(zp)
        out[f"vwall{q}_paths"] = np.array(list(zip(*lists)), dtype=np.float64).reshape(-1, 4)
        out[f"vwall{q}_ncoll"] = np.int64(counter.value)
    # side walls: particles just outside radius R moving outward (as after a drift step)
    radii = [(float(P.open_air_radius), float(P.open_air_collision_radius)),
             (float(P.gap_radius), float(P.gap_collision_radius)),
             (float(P.pore_coated_radius), float(P.pore_collision_radius))]
    for q, (R, Rc) in enumerate(radii):
        st = set_state(nw)
        # start strictly inside Rc, fly along v until r = R*(1+eps): the back-solve then always has real roots
        th = rng.uniform(0, 2 * np.pi, nw)
        r0 = Rc * rng.uniform(0.3, 0.999, nw)
        x0, y0 = r0 * np.cos(th), r0 * np.sin(th)
        vx, vy = rng.normal(size=nw) * 249.0, rng.normal(size=nw) * 249.0
        rt = R * (1 + rng.uniform(1e-6, 3e-3, nw))
        qa, qb, qc = vx * vx + vy * vy, 2 * (x0 * vx + y0 * vy), x0 * x0 + y0 * y0 - rt * rt
        s = (-qb + np.sqrt(qb * qb - 4 * qa * qc)) / (2 * qa)
        st["x_vals"] = x0 + vx * s
        st["y_vals"] = y0 + vy * s
        st["x_velocities"] = vx
        st["y_velocities"] = vy
        hits = rng.random(nw) < 0.5
        load(st)
        counter = multiprocessing.Value('i', 0)
        P.num_collisions_per_step = counter
        lists = [[], [], [], []]
        P.hit_cylinder_side_wall(hits, Rc, *lists)
        res = grab()
        for k in STATE_KEYS:
            out[f"swall{q}_in_{k}"] = st[k]
            out[f"swall{q}_out_{k}"] = res[k]
        out[f"swall{q}_hits"] = hits
        out[f"swall{q}_Rc"] = np.float64(Rc)
        out[f"swall{q}_paths"] = np.array(list(zip(*lists)), dtype=np.float64).reshape(-1, 4)
        out[f"swall{q}_ncoll"] = np.int64(counter.value)

    # --- (iv) the mutating bounds check -------------------------------------------------------------------
    st = set_state(4000)
    st["x_vals"] *= 1.2
    load(st)
    cnt = P.num_out_of_bounds()
    res = grab()
    for k in ["x_vals", "y_vals", "z_vals"]:
        out[f"oob_in_{k}"] = st[k]
        out[f"oob_out_{k}"] = res[k]
    out["oob_count"] = np.int64(cnt)

    # --- SURVEY 8c known-answer vector ------------------------------------------------------------------------
    counter = multiprocessing.Value('i', 0)
    P.init_globals(counter)
    lists = [[], [], [], []]
    res = P.pairwise_particles_in_cell(*lists, np.array([True, True]), np.array([1e-8, 2e-8]), np.array([1e-8, 2e-8]),
                                       np.zeros(2), np.zeros(2), np.array([True, False]), np.array([0.0, 0.9 * cr]),
                                       np.zeros(2), np.zeros(2), np.array([100.0, -100.0]), np.zeros(2), np.zeros(2))
    out["kat_x"] = res[6]
    out["kat_vx"] = res[9]
    out["kat_cont"] = res[1]
    out["kat_paths"] = np.array([lists[0][0], lists[1][0], lists[2][0], lists[3][0]])

    np.savez_compressed(os.path.join(OUT, "func_pore.npz"), **out)
    print("func_pore.npz:", len(out), "arrays")


# ------------------------------------------------------------------------------------------------ edge inputs
EDGE_PLANES = ("zero", "H", "z_cold", "h_oa", "z_gap_bottom", "z_gap_top")


def edge_side_cases():
    """(case-name prefix, which collision radius) of the side-wall solves in tests/edge_states.pore_walls"""
    return (("tangent_", "R_oa_c"), ("side_a0", "R_oa_c"), ("cur_r_R_oa", "R_oa_c"), ("graze_Rg", "R_g_c"),
            ("cur_r_R_g", "R_g_c"), ("corner_Rg", "R_g_c"), ("graze_Rp", "R_p_c"), ("cur_r_R_p", "R_p_c"),
            ("corner_Rp", "R_p_c"))


def edge_inputs():
    """The inputs of --only edge, built from tests/edge_states.py (also used by tests/test_oracle_edges.py to check that
    the fixture still belongs to the builders)."""
    sys.path.insert(0, os.path.dirname(HERE))
    from tests import edge_states as E
    w = E.pore_walls(fp_cases=True)
    p = w.p
    dt = w.dt
    # the positions and accumulators after the drift (ndarray arithmetic, Pore:427-437)
    st = {}
    for k, v in zip(STATE_KEYS[:3], (w.x, w.y, w.z)):
        st[k] = v.copy()
    sx, sy, sz = dt * w.vx, dt * w.vy, dt * w.vz
    st["x_vals"], st["y_vals"], st["z_vals"] = w.x + sx, w.y + sy, w.z + sz
    st["x_velocities"], st["y_velocities"], st["z_velocities"] = w.vx.copy(), w.vy.copy(), w.vz.copy()
    st["dist_since_collision"] = w.d + np.abs(np.sqrt(sx * sx + sy * sy + sz * sz))
    st["dist_x_since_collision"], st["dist_y_since_collision"] = w.dx + np.abs(sx), w.dy + np.abs(sy)
    st["dist_z_since_collision"] = w.dz + np.abs(sz)
    st["full_path_traveled"] = w.flag.astype(bool)
    out = {"wall_in_" + k: v for k, v in st.items()}
    planes = dict(zero=0.0, H=p.H, z_cold=p.z_cold, h_oa=p.h_oa, z_gap_bottom=p.z_gap_bottom, z_gap_top=p.z_gap_top)
    for q, name in enumerate(EDGE_PLANES):
        hits = np.zeros(w.n, dtype=bool)
        for case in (f"cur_z_{name}", f"prior_z_{name}"):
            hits[w.cases[case]] = True
        # (not here: vz == 0 on the plane is 0 / 0, and the smallest |vz| underflows in vz**2 — the reference raises on
        # both under np.seterr(all='raise'))
        out[f"vedge{q}_hits"] = hits
        out[f"vedge{q}_plane"] = np.float64(planes[name])
    side = []
    for pre, rc in edge_side_cases():
        for case, idx in w.cases.items():
            if case.startswith(pre):
                side += [(i, getattr(p, rc)) for i in idx]
    out["sedge_idx"] = np.array([i for i, _ in side], dtype=np.int64)
    out["sedge_Rc"] = np.array([r for _, r in side], dtype=np.float64)
    b = E.pore_bounds()
    out["bedge_in_x"], out["bedge_in_y"], out["bedge_in_z"] = b.x, b.y, b.z
    # pairs around collision_range (the detection-grid pairs, positions as built)
    fields = ["cont", "cx", "cy", "cz", "flag", "x", "y", "z", "vx", "vy", "vz"]
    pin = {f: [] for f in fields}
    for kind in ("pore", "cube"):
        g = E.grid_pairs(kind, for_timestep=False)
        for i, j in g.extra["pairs"]:
            s = [i, j]
            for f, a in zip(fields, (g.d[s], g.dx[s], g.dy[s], g.dz[s], g.flag[s].astype(bool), g.x[s], g.y[s], g.z[s],
                                     g.vx[s], g.vy[s], g.vz[s])):
                pin[f].append(np.asarray(a, dtype=np.float64))
    for f in fields:
        out["pedge_in_" + f] = np.array(pin[f])
    return out


def gen_edge():
    """The reference's own wall, bounds and pair functions on the crafted edge inputs (tests/edge_states.py)."""
    out = edge_inputs()                 # (before the import: the reference turns every floating-point warning into an error)
    os.environ.setdefault("MPLBACKEND", "Agg")
    sys.path.insert(0, REF)
    import multiprocessing
    import Open_Air_Pore_MC as P  # noqa

    wst = {k: out["wall_in_" + k] for k in STATE_KEYS}

    def load(st):
        for k, v in st.items():
            setattr(P, k, v.copy())

    def grab():
        return {k: getattr(P, k).copy() for k in STATE_KEYS}

    for q in range(len(EDGE_PLANES)):
        load(wst)
        counter = multiprocessing.Value('i', 0)
        P.num_collisions_per_step = counter
        lists = [[], [], [], []]
        P.hit_vertical_wall(out[f"vedge{q}_hits"], float(out[f"vedge{q}_plane"]), *lists)
        res = grab()
        for k in STATE_KEYS:
            out[f"vedge{q}_out_{k}"] = res[k]
        out[f"vedge{q}_paths"] = np.array(list(zip(*lists)), dtype=np.float64).reshape(-1, 4)
        out[f"vedge{q}_ncoll"] = np.int64(counter.value)
    # side walls one particle at a time: a solve without a real root ends the reference's call (its except branch
    # raises), so only the outcome is kept for those
    ns = len(out["sedge_idx"])
    outcome = np.zeros(ns, dtype=np.int64)
    sout = {k: np.zeros(ns) for k in STATE_KEYS}
    spaths = np.full((ns, 4), np.nan)
    for m, (i, Rc) in enumerate(zip(out["sedge_idx"], out["sedge_Rc"])):
        load({k: v[i:i + 1] for k, v in wst.items()})
        counter = multiprocessing.Value('i', 0)
        P.num_collisions_per_step = counter
        lists = [[], [], [], []]
        try:
            P.hit_cylinder_side_wall(np.array([True]), float(Rc), *lists)
        except Exception:          # (UnboundLocalError from the except branch's `total_errs += 1`)
            outcome[m] = 1
            for k in STATE_KEYS:
                sout[k][m] = wst[k][i]
            continue
        res = grab()
        for k in STATE_KEYS:
            sout[k][m] = res[k][0]
        if lists[0]:
            spaths[m] = [lists[0][0], lists[1][0], lists[2][0], lists[3][0]]
    out["sedge_outcome"] = outcome
    out["sedge_paths"] = spaths
    for k in STATE_KEYS:
        out[f"sedge_out_{k}"] = sout[k]
    # the mutating bounds check
    n = len(out["bedge_in_x"])
    load({"x_vals": out["bedge_in_x"], "y_vals": out["bedge_in_y"], "z_vals": out["bedge_in_z"]})
    out["bedge_count"] = np.int64(P.num_out_of_bounds())
    for k, f in (("x_vals", "x"), ("y_vals", "y"), ("z_vals", "z")):
        out[f"bedge_out_{f}"] = getattr(P, k).copy()
    assert len(out["bedge_out_x"]) == n
    # pairs around collision_range
    fields = ["cont", "cx", "cy", "cz", "flag", "x", "y", "z", "vx", "vy", "vz"]
    npair = out["pedge_in_x"].shape[0]
    pout = {f: np.zeros((npair, 2)) for f in fields}
    ppaths = np.full((npair, 2, 4), np.nan)
    pnc = np.zeros(npair, dtype=np.int64)
    for k in range(npair):
        counter = multiprocessing.Value('i', 0)
        P.init_globals(counter)
        args = [out["pedge_in_" + f][k].copy() for f in fields]
        args[4] = args[4].astype(bool)
        lists = [[], [], [], []]
        res = P.pairwise_particles_in_cell(*lists, np.array([True, True]), *args)
        for f, a in zip(fields, res[1:]):
            pout[f][k] = a
        for q in range(len(lists[0])):
            ppaths[k, q] = [lists[0][q], lists[1][q], lists[2][q], lists[3][q]]
        pnc[k] = counter.value
    for f in fields:
        out["pedge_out_" + f] = pout[f]
    out["pedge_paths"] = ppaths
    out["pedge_ncoll"] = pnc
    np.savez_compressed(os.path.join(OUT, "func_edge.npz"), **out)
    print("func_edge.npz:", len(out), "arrays,", int(outcome.sum()), "side-wall solves without a real root,",
          int(pnc.sum()), "pair collisions")


# ------------------------------------------------------------------------------------------------ crafted clusters
CLUSTER_FIELDS = ["cont", "cx", "cy", "cz", "flag", "x", "y", "z", "vx", "vy", "vz"]
CLUSTER_PERMS = ("identity", "reversed")


def cluster_inputs():
    """The inputs of --only clusters, built from tests/cluster_states.py: every cluster of every catalogue state (pore
    geometry; the 80 copies of items_over / items_fit are left out, pair_pull1 has them already) as ONE cell — the
    particles of its site in ascending index, positions and accumulators after the drift (Pore:427-437) — under the
    identity and the reversed permutation."""
    sys.path.insert(0, os.path.dirname(HERE))
    from tests import cluster_states as CS
    cells, names = {f: [] for f in CLUSTER_FIELDS}, []
    off = [0]
    for perm in CLUSTER_PERMS:
        for which in ("within",) + CS.HANDOVER:
            s = CS.catalogue("pore", perm, which)
            sx, sy, sz = s.dt * s.vx, s.dt * s.vy, s.dt * s.vz
            st = dict(cont=s.d + np.abs(np.sqrt(sx * sx + sy * sy + sz * sz)), cx=s.dx + np.abs(sx), cy=s.dy + np.abs(sy),
                      cz=s.dz + np.abs(sz), flag=s.flag.astype(np.float64), x=s.x + sx, y=s.y + sy, z=s.z + sz,
                      vx=s.vx, vy=s.vy, vz=s.vz)
            site = s.extra["site"]
            case_of = np.empty(s.n, dtype=object)
            for case, idx in s.cases.items():
                case_of[idx] = case
            for q in range(int(site.max()) + 1):
                idx = np.flatnonzero(site == q)         # (ascending particle index)
                if which != "within" and case_of[idx[0]] == "pair":
                    continue                            # (the company of a hand-over state: `within` has that pair)
                for f in CLUSTER_FIELDS:
                    cells[f].append(st[f][idx])
                names.append(f"{perm}/{case_of[idx[0]]}")
                off.append(off[-1] + len(idx))
    out = {"cl_in_" + f: np.concatenate(cells[f]) for f in CLUSTER_FIELDS}
    out["cl_off"] = np.array(off, dtype=np.int64)
    out["cl_name"] = np.array(names, dtype="U40")
    return out


def gen_clusters():
    """The reference's own pairwise_particles_in_cell on the crafted clusters (tests/cluster_states.py), one cell each."""
    out = cluster_inputs()              # (before the import: the reference turns every floating-point warning into an error)
    os.environ.setdefault("MPLBACKEND", "Agg")
    sys.path.insert(0, REF)
    import multiprocessing
    import Open_Air_Pore_MC as P  # noqa
    off = out["cl_off"]
    ncell = len(off) - 1
    res_all = {f: out["cl_in_" + f].copy() for f in CLUSTER_FIELDS}
    paths, path_off = [], [0]
    ncoll = np.zeros(ncell, dtype=np.int64)
    outcome = np.zeros(ncell, dtype=np.int64)
    for c in range(ncell):
        sl = slice(int(off[c]), int(off[c + 1]))
        counter = multiprocessing.Value('i', 0)
        P.init_globals(counter)
        args = [out["cl_in_" + f][sl].copy() for f in CLUSTER_FIELDS]
        args[4] = args[4].astype(bool)
        lists = [[], [], [], []]
        try:
            res = P.pairwise_particles_in_cell(*lists, np.ones(sl.stop - sl.start, dtype=bool), *args)
        except FloatingPointError:      # (equal velocities: a == 0 in the contact solve ends the reference's run)
            outcome[c] = 1
            path_off.append(len(paths))
            continue
        for f, a in zip(CLUSTER_FIELDS, res[1:]):
            res_all[f][sl] = np.asarray(a, dtype=np.float64)
        paths.extend(zip(*lists))
        path_off.append(len(paths))
        ncoll[c] = counter.value
    for f in CLUSTER_FIELDS:
        out["cl_out_" + f] = res_all[f]
    out["cl_paths"] = np.array(paths, dtype=np.float64).reshape(-1, 4)
    out["cl_path_off"] = np.array(path_off, dtype=np.int64)
    out["cl_ncoll"] = ncoll
    out["cl_outcome"] = outcome
    save_npz_deterministic(os.path.join(OUT, "func_clusters.npz"), out)
    print("func_clusters.npz:", ncell, "cells,", int(ncoll.sum()), "collisions,", int(outcome.sum()), "cells the reference raised on")


# ------------------------------------------------------------------------------------------------ ordered-workgroup cells
def resolve_inputs():
    """The inputs of --only resolve, built from tests/resolve_states.py: its family-A cells of up to a few hundred particles
    (the split / pool fences, the head and coop cells, the merging clusters, short cascades), each as ONE cell."""
    sys.path.insert(0, os.path.dirname(HERE))
    from tests import resolve_states as RS
    cells = [RS.cell(name) for name in RS.SMALL]
    out = {"rs_in_" + f: np.concatenate([np.asarray(c.arrays[f], dtype=np.float64) for c in cells]) for f in CLUSTER_FIELDS}
    out["rs_off"] = np.cumsum([0] + [c.n for c in cells]).astype(np.int64)
    out["rs_name"] = np.array(RS.SMALL, dtype="U40")
    return out


def gen_resolve():
    """The reference's own pairwise_particles_in_cell on the crafted cells of tests/resolve_states.py."""
    out = resolve_inputs()              # (before the import: the reference turns every floating-point warning into an error)
    os.environ.setdefault("MPLBACKEND", "Agg")
    sys.path.insert(0, REF)
    import multiprocessing
    import Open_Air_Pore_MC as P  # noqa
    off = out["rs_off"]
    ncell = len(off) - 1
    res_all = {f: out["rs_in_" + f].copy() for f in CLUSTER_FIELDS}
    paths, path_off = [], [0]
    ncoll = np.zeros(ncell, dtype=np.int64)
    for c in range(ncell):
        sl = slice(int(off[c]), int(off[c + 1]))
        counter = multiprocessing.Value('i', 0)
        P.init_globals(counter)
        args = [out["rs_in_" + f][sl].copy() for f in CLUSTER_FIELDS]
        args[4] = args[4].astype(bool)
        lists = [[], [], [], []]
        res = P.pairwise_particles_in_cell(*lists, np.ones(sl.stop - sl.start, dtype=bool), *args)
        for f, a in zip(CLUSTER_FIELDS, res[1:]):
            res_all[f][sl] = np.asarray(a, dtype=np.float64)
        paths.extend(zip(*lists))
        path_off.append(len(paths))
        ncoll[c] = counter.value
    for f in CLUSTER_FIELDS:
        out["rs_out_" + f] = res_all[f]
    out["rs_paths"] = np.array(paths, dtype=np.float64).reshape(-1, 4)
    out["rs_path_off"] = np.array(path_off, dtype=np.int64)
    out["rs_ncoll"] = ncoll
    save_npz_deterministic(os.path.join(OUT, "func_resolve.npz"), out)
    print("func_resolve.npz:", ncell, "cells,", int(ncoll.sum()), "collisions")


# ------------------------------------------------------------------------------------------------ constants
def gen_consts():
    """Module constants of the three scripts, captured from the reference's own evaluation."""
    os.environ.setdefault("MPLBACKEND", "Agg")
    sys.path.insert(0, REF)
    import Open_Air_Pore_MC as P  # noqa
    import Temperature_Pore_MC as T  # noqa
    names = ["pore_coated_radius", "gap_radius", "pore_height", "hot_coating_height", "gap_height",
             "cold_coating_height", "open_air_radius", "open_air_height", "total_volume", "total_height", "dx", "dy",
             "dz", "argon_mass", "argon_radius", "collision_range", "lambda_mfp", "v_mean", "a_shape", "num_molecules",
             "open_air_collision_radius", "gap_collision_radius", "pore_collision_radius", "tau", "dt",
             "open_air_particles", "cold_pore_particles", "hot_pore_particles", "gap_particles", "remaining_particles"]
    out = {}
    for mod, tag in ((P, "pore"), (T, "temp")):
        for k in names:
            out[f"{tag}_{k}"] = np.float64(getattr(mod, k))
    out["pore_z_gap_top_expr"] = np.float64(P.total_height - P.open_air_height - P.cold_coating_height)
    out["pore_z_gap_bottom_expr"] = np.float64(P.open_air_height + P.hot_coating_height)
    out["temp_gap_bottom_height"] = np.float64(T.gap_bottom_height)
    out["temp_gap_top_height"] = np.float64(T.gap_top_height)
    out["temp_surface_energy_cold"] = np.float64(float(T.surface_energy_cold))
    out["temp_surface_energy_hot"] = np.float64(float(T.surface_energy_hot))
    out["temp_R_g_c_sq"] = np.float64(T.gap_collision_radius ** 2)
    out["temp_R_p_c_sq"] = np.float64(T.pore_collision_radius ** 2)
    out["pore_R_oa_sq"] = np.float64(P.open_air_radius ** 2)
    out["pore_R_g_sq"] = np.float64(P.gap_radius ** 2)
    out["pore_R_p_sq"] = np.float64(P.pore_coated_radius ** 2)
    # Cube cannot be imported without running its simulation: evaluate only its constant block (the lines before
    # the RNG seeding) in a scratch namespace
    src = open(os.path.join(REF, "Open_Air_Cube_MC.py")).read().split("\n")
    end = next(i for i, l in enumerate(src) if l.startswith("np.random.seed"))
    ns = {}
    block = "\n".join(l for l in src[:end] if not l.startswith("print("))
    exec(compile(block, "<cube-constants>", "exec"), ns)
    for k in ["cube_x", "dx", "collision_x_overlap", "argon_radius", "collision_range", "lambda_mfp", "v_mean",
              "a_shape", "num_molecules", "tau", "dt", "num_timesteps"]:
        out[f"cube_{k}"] = np.float64(ns[k])
    np.savez_compressed(os.path.join(OUT, "consts.npz"), **out)
    print("consts.npz:", len(out), "values")


# ------------------------------------------------------------------------------------------------ step level
HOOK = r'''
import sys, numpy as np
_KEYS = %r
_snap_steps = set(%r)
_hash_all = %r
_store = {}
_prev = {}
def dump(step, ncoll=None, lists=None):
    m = sys.modules['__main__']
    g = m.__dict__
    def arr(k):
        a = np.asarray(g[k])
        return a.reshape(-1).copy()
    if step in _snap_steps:
        for k in _KEYS:
            _store['s%%04d_%%s' %% (step, k)] = arr(k)
    if _hash_all:
        # natural-size runs: SHA-256 of every state array after every step instead of the arrays (49 MB per snapshot at
        # N = 557,649), plus the indices of the particles whose velocity changed in the step (the step's event set)
        import hashlib
        ch = None
        for k in _KEYS:
            a = arr(k)
            a = a.astype(np.uint8) if a.dtype == bool else np.ascontiguousarray(a, dtype=np.float64)
            _store['h%%04d_%%s' %% (step, k)] = np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8)
            if k.endswith('_velocities'):
                if k in _prev:
                    d = a != _prev[k]
                    ch = d if ch is None else (ch | d)
                _prev[k] = a
        if ch is not None:
            _store['ev%%04d' %% step] = np.nonzero(ch)[0].astype(np.int32)
    if step == -1:
        import random as _r
        st = np.random.get_state()
        _store['rng_np_keys'] = np.asarray(st[1], dtype=np.uint32)
        _store['rng_np_pos'] = np.int64(st[2])
        _store['rng_np_gauss'] = np.array([st[3], st[4]], dtype=np.float64)
        ps = _r.getstate()
        _store['rng_py_state'] = np.asarray(ps[1], dtype=np.uint64)
        _store['rng_py_version'] = np.int64(ps[0])
    st = _store.setdefault('per_step', [])
    if step >= 0:
        vx, vy, vz = arr('x_velocities'), arr('y_velocities'), arr('z_velocities')
        st.append([step, -1 if ncoll is None else int(ncoll), -1 if lists is None else len(lists[0]),
                   float(np.sum(arr('x_vals'))), float(np.sum(arr('y_vals'))), float(np.sum(arr('z_vals'))),
                   float(np.sum(vx)), float(np.sum(vy)), float(np.sum(vz)), float(np.sum(vx*vx+vy*vy+vz*vz)),
                   float(np.sum(arr('dist_since_collision'))), float(np.sum(arr('full_path_traveled')))])
def load_state(path):
    # crafted inputs (tests/edge_states.py) in place of the script's own initial state: its arrays are module globals
    g = sys.modules['__main__'].__dict__
    with np.load(path) as d:
        for k in _KEYS:
            assert g[k].shape == d[k].shape and g[k].dtype == d[k].dtype, k
            g[k] = d[k].copy()
def dump_cases(masks, scalars, lists):
    # after the last energised case of a step: the masks by their names in the script, the state, the sums, the paths
    g = sys.modules['__main__'].__dict__
    for k in masks:
        _store['c_' + k] = np.asarray(g[k]).astype(bool).copy()
    for k in _KEYS:
        _store['c_' + k] = np.asarray(g[k]).reshape(-1).copy()
    for k, v in scalars.items():
        _store['c_' + k] = np.asarray(v)
    _store['c_paths'] = np.array([list(l) for l in lists], dtype=np.float64).reshape(4, -1).T.copy()
def finish(lists, extra=None):
    _store['per_step'] = np.array(_store.get('per_step', []), dtype=np.float64).reshape(-1, 12)
    for name, l in zip(['completed_paths', 'completed_x_paths', 'completed_y_paths', 'completed_z_paths'], lists):
        _store[name] = np.array(list(l), dtype=np.float64)
    if extra:
        for k, v in extra.items():
            _store[k] = np.asarray(v)
    np.savez_compressed('golden_dump.npz', **_store)
'''


def _patch_lines(lines, subs):
    """subs: list of (regex matching a whole source line, replacement-or-callable).  Each must hit exactly once."""
    for pat, rep in subs:
        idx = [i for i, l in enumerate(lines) if re.match(pat, l)]
        if len(idx) != 1:
            raise RuntimeError(f"pattern {pat!r} matched {len(idx)} lines")
        i = idx[0]
        lines[i] = rep(lines[i]) if callable(rep) else rep
    return lines


def _indent_of(line):
    return line[:len(line) - len(line.lstrip())]


def save_npz_deterministic(path, arrays):
    """np.savez_compressed with fixed member times and order: the same arrays give the same bytes on every run"""
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            with z.open(info, "w") as fh:
                np.lib.format.write_array(fh, np.asanyarray(arrays[k]), allow_pickle=False)


def run_patched(script, subs, inserts, snap_steps, out_name, meta, timeout=3600, hash_all=False, files=None, keep_text=True,
                post=None):
    """inserts: list of (regex of anchor line, 'before'|'after', code string using the anchor's indentation).
    files: {name: {key: array}} written as .npz beside the patched script; post(d): last word on the dump, which is then
    written with fixed member times (byte-identical from run to run)."""
    work = tempfile.mkdtemp(prefix="amc_golden_", dir="/tmp")
    try:
        lines = open(os.path.join(REF, script)).read().split("\n")
        lines = _patch_lines(lines, subs)
        for pat, where, code in inserts:
            idx = [i for i, l in enumerate(lines) if re.match(pat, l)]
            if len(idx) != 1:
                raise RuntimeError(f"anchor {pat!r} matched {len(idx)} lines")
            i = idx[0]
            ind = _indent_of(lines[i])
            new = [ind + c for c in code.split("\n")]
            lines[i + 1:i + 1] = new if where == "after" else []
            if where == "before":
                lines[i:i] = new
        lines.insert(0, "import _golden_hook")
        with open(os.path.join(work, "patched.py"), "w") as f:
            f.write("\n".join(lines))
        with open(os.path.join(work, "_golden_hook.py"), "w") as f:
            f.write(HOOK % (STATE_KEYS, sorted(snap_steps), bool(hash_all)))
        shutil.copy(os.path.join(REF, "utils.py"), os.path.join(work, "utils.py"))
        for name, arrays in (files or {}).items():
            np.savez(os.path.join(work, name), **arrays)
        env = dict(os.environ, MPLBACKEND="Agg", PYTHONDONTWRITEBYTECODE="1")
        r = subprocess.run([sys.executable, "-u", "patched.py"], cwd=work, env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, timeout=timeout)
        tail = r.stdout.decode(errors="replace")[-3000:]
        if r.returncode != 0:
            print(tail)
            raise RuntimeError(f"{script} patched run failed rc={r.returncode}")
        d = dict(np.load(os.path.join(work, "golden_dump.npz")))
        for k, v in meta.items():
            d["meta_" + k] = np.asarray(v)
        # the text outputs the script wrote (format goldens)
        for fn in sorted(os.listdir(work)) if keep_text else ():
            if fn.startswith("hist_") and fn.endswith(".txt") or fn == "momentum_energy.csv":
                d["file_" + fn] = np.frombuffer(open(os.path.join(work, fn), "rb").read(), dtype=np.uint8)
        if post is not None:
            post(d)
            save_npz_deterministic(os.path.join(OUT, out_name), d)
        else:
            np.savez_compressed(os.path.join(OUT, out_name), **d)
        print(out_name, "written;", "steps:", d["per_step"].shape[0], "paths:",
              (d["completed_paths"] if "completed_paths" in d else d["completed_rows"]).shape[0])
    finally:
        shutil.rmtree(work, ignore_errors=True)


def gen_pore(tag, K, sigma_mult, slice_, steps, snaps):
    subs = [
        (r"^num_molecules\s+= np\.round\(", f"num_molecules       = np.int64({K})"),
        (r"^sigma\s+= 3\.6", f"sigma               = 3.6 * 10**(-19) * {sigma_mult}"),
        (r"^NMFT_slice\s+= 1000", f"NMFT_slice          = {slice_}"),
        (r"^        for i in range\(num_timesteps\):", f"        for i in range({steps}):"),
    ]
    inserts = [
        (r"^        for i in range\(\d+\):", "before", "_golden_hook.dump(-1)"),
        (r"^            print\('   ',num_collisions_per_step\.value,' collisions from this timestep'\)", "after",
         "_golden_hook.dump(i, num_collisions_per_step.value, [completed_paths])"),
        (r"^        print\('Num of measured full paths total: '", "after",
         "_golden_hook.finish([completed_paths, completed_x_paths, completed_y_paths, completed_z_paths], "
         "dict(dt=dt, collision_range=collision_range, total_cols=total_cols))"),
    ]
    run_patched("Open_Air_Pore_MC.py", subs, inserts, set(snaps) | {-1},
                f"step_pore_{tag}.npz", dict(K=K, sigma_mult=sigma_mult, slice=slice_, steps=steps))


def gen_temp(tag, K, sigma_mult, slice_, steps, snaps):
    subs = [
        (r"^num_molecules\s+= np\.round\(", f"num_molecules               = np.int64({K})"),
        (r"^sigma\s+= 3\.6", f"sigma                       = 3.6 * 10**(-19) * {sigma_mult}"),
        (r"^nmft_slice\s+= 1000", f"nmft_slice                  = {slice_}"),
        (r"^        for step in range\(num_timesteps\):", f"        for step in range({steps}):"),
    ]
    inserts = [
        (r"^        for step in range\(\d+\):", "before", "_golden_hook.dump(-1)"),
        (r"^            print\('   ',num_collisions_per_step\.value,' collisions from this timestep'\)", "after",
         "_golden_hook.dump(step, num_collisions_per_step.value, [completed_paths])"),
        (r"^        print\('Num of measured full paths total: '", "after",
         "_golden_hook.finish([completed_paths, completed_x_paths, completed_y_paths, completed_z_paths], "
         "dict(dt=dt, collision_range=collision_range, total_cols=total_cols, total_errs=total_errs, "
         "momentum=[float(v) for v in momentum_z_change_per_step], "
         "energy_cold=[float(v) for v in energy_transfer_cold_per_step], "
         "energy_hot=[float(v) for v in energy_transfer_hot_per_step]))"),
    ]
    run_patched("Temperature_Pore_MC.py", subs, inserts, set(snaps) | {-1},
                f"step_temp_{tag}.npz", dict(K=K, sigma_mult=sigma_mult, slice=slice_, steps=steps))


TEMP_MASKS = {3: "hit_vertical_int_open_air_cold", 4: "hit_vertical_int_open_air_hot", 5: "hit_gap_cylinder_wall",
              6: "hit_gap_cylinder_base_bottom", 7: "hit_gap_cylinder_base_top", 8: "hit_pore_coating_hot",
              9: "hit_pore_coating_cold"}        # case id -> the mask's name in Temperature_Pore_MC.py (Temp:708-749)


def temp_edge_inputs():
    """The inputs of --only temp_edge: tests/edge_states.temp_walls(reference_safe=True) under the reference's names (also
    used by tests/test_oracle_edges.py to check that the fixture still belongs to the builder)."""
    sys.path.insert(0, os.path.dirname(HERE))
    from tests import edge_states as E
    w = E.temp_walls(reference_safe=True)
    a = w.arrays()
    st = {k: v for k, v in zip(STATE_KEYS[:10], a[:10])}
    st["full_path_traveled"] = a[10].astype(bool)
    return st


def gen_temp_edge():
    """Temperature_Pore_MC.py for ONE step on the crafted energised edge state: its own masks (inline in its main loop, so
    no function-level fixture reaches them), the state after the seven cases and after the step, its error count, paths
    and sums.  num_molecules is the state's size; the state arrays are overwritten just before the time loop."""
    st = temp_edge_inputs()
    n = len(st["x_vals"])
    subs = [
        (r"^num_molecules\s+= np\.round\(", f"num_molecules               = np.int64({n})"),
        (r"^        for step in range\(num_timesteps\):", "        for step in range(1):"),
    ]
    names = [TEMP_MASKS[k] for k in sorted(TEMP_MASKS)]
    inserts = [
        (r"^        for step in range\(\d+\):", "before", "_golden_hook.load_state('edge_state.npz')"),
        (r"^        for step in range\(\d+\):", "before", "_golden_hook.dump(-1)"),
        (r"^            energy_transfer_cold_per_step\.append\(energy_change_cold_in_step\)", "after",
         f"_golden_hook.dump_cases({names!r}, dict(total_errs=total_errs, "
         "momentum_z_change_in_step=float(momentum_z_change_in_step), "
         "energy_change_cold_in_step=float(energy_change_cold_in_step), "
         "energy_change_hot_in_step=float(energy_change_hot_in_step)), "
         "[completed_paths, completed_x_paths, completed_y_paths, completed_z_paths])"),
        (r"^            print\('   ',num_collisions_per_step\.value,' collisions from this timestep'\)", "after",
         "_golden_hook.dump(step, num_collisions_per_step.value, [completed_paths])"),
        (r"^        print\('Num of measured full paths total: '", "after",
         "_golden_hook.finish([completed_paths, completed_x_paths, completed_y_paths, completed_z_paths], "
         "dict(dt=dt, collision_range=collision_range, total_cols=total_cols, total_errs=total_errs))"),
    ]

    def post(d):
        # the sweep's workers append their paths in scheduling order: store the rows sorted (they are compared as a multiset)
        rows = np.stack([d.pop("completed_paths"), d.pop("completed_x_paths"), d.pop("completed_y_paths"),
                         d.pop("completed_z_paths")], axis=1)
        d["completed_rows"] = rows[np.lexsort(rows.T[::-1])]
        for k in TEMP_MASKS.values():
            d["c_" + k] = np.packbits(d["c_" + k])

    run_patched("Temperature_Pore_MC.py", subs, inserts, {-1, 0}, "func_temp_edge.npz", dict(K=n, steps=1),
                files={"edge_state.npz": st}, keep_text=False, post=post)


def gen_cube(tag, K, sigma_mult, steps, snaps):
    subs = [
        (r"^num_molecules\s+= np\.round\(", f"num_molecules       = np.int64({K})"),
        (r"^sigma\s+= 3\.6", f"sigma               = 3.6 * 10**(-19) * {sigma_mult}"),
        (r"^    for i in range\(num_timesteps\):", f"    for i in range({steps}):"),
    ]
    inserts = [
        (r"^    for i in range\(\d+\):", "before", "_step = -1\n_golden_hook.dump(-1)"),
        (r"^        print\('  timestep',i,'of',num_timesteps", "before", "_step += 1"),
        (r"^        print\('    ',N_collisions,' collisions'\)", "after",
         "_golden_hook.dump(_step, N_collisions, [completed_paths[sim]])"),
        (r"^    #generate figure for graphing", "before",
         "_golden_hook.finish([completed_paths[sim], completed_x_paths[sim], completed_y_paths[sim], "
         "completed_z_paths[sim]], dict(dt=dt, collision_range=collision_range))\nraise SystemExit(0)"),
    ]
    run_patched("Open_Air_Cube_MC.py", subs, inserts, set(snaps) | {-1},
                f"step_cube_{tag}.npz", dict(K=K, sigma_mult=sigma_mult, steps=steps))


def gen_cube_natural(steps=30):
    """Open_Air_Cube_MC.py AS WRITTEN (N = 24,627, sigma x 1, dt = tau / 25) except the loop bound and the dump hook:
    initial state in full, then per step the counters, the SHA-256 of every state array and the event set."""
    subs = [(r"^    for i in range\(num_timesteps\):", f"    for i in range({steps}):")]
    inserts = [
        (r"^    for i in range\(\d+\):", "before", "_step = -1\n_golden_hook.dump(-1)"),
        (r"^        print\('  timestep',i,'of',num_timesteps", "before", "_step += 1"),
        (r"^        print\('    ',N_collisions,' collisions'\)", "after",
         "_golden_hook.dump(_step, N_collisions, [completed_paths[sim]])"),
        (r"^    #generate figure for graphing", "before",
         "_golden_hook.finish([completed_paths[sim], completed_x_paths[sim], completed_y_paths[sim], "
         "completed_z_paths[sim]], dict(dt=dt, collision_range=collision_range, num_molecules=num_molecules))\nraise SystemExit(0)"),
    ]
    run_patched("Open_Air_Cube_MC.py", subs, inserts, {-1}, "step_cube_natural.npz",
                dict(K=-1, sigma_mult=1, steps=steps, natural=1), hash_all=True)


def gen_pore_natural(steps=3):
    """Open_Air_Pore_MC.py AS WRITTEN (N = 557,649, sigma = 3.6e-19, its own initial conditions from np.random.seed(17) /
    seed(17)) except the loop bound and the dump hook.  The initial state is NOT stored (27 MB of random doubles): its
    SHA-256 is, and tests/natural_ic.py regenerates it from the same seeds with the same library calls (the recipe is
    checked against the hashes before anything is compared).  About a minute per step in the build container."""
    subs = [(r"^        for i in range\(num_timesteps\):", f"        for i in range({steps}):")]
    inserts = [
        (r"^        for i in range\(\d+\):", "before", "_golden_hook.dump(-1)"),
        (r"^            print\('   ',num_collisions_per_step\.value,' collisions from this timestep'\)", "after",
         "_golden_hook.dump(i, num_collisions_per_step.value, [completed_paths])"),
        (r"^        print\('Num of measured full paths total: '", "after",
         "_golden_hook.finish([completed_paths, completed_x_paths, completed_y_paths, completed_z_paths], "
         "dict(dt=dt, collision_range=collision_range, total_cols=total_cols, num_molecules=num_molecules))"),
    ]
    run_patched("Open_Air_Pore_MC.py", subs, inserts, set(), "step_pore_natural.npz",
                dict(K=-1, sigma_mult=1, slice=1000, steps=steps, natural=1), hash_all=True, timeout=7200)


def gen_graph_hist():
    """The one physics artefact the reference holds: the 200-bin cube free-path histogram pasted into graph_sim_data.py
    (x_data = bin left edges, y_data = density over 423,143 paths).  Only the two arrays are taken — evaluated from the
    two assignments, nothing else of the script is run — plus the exponential fit the script itself performs on them."""
    from scipy.optimize import curve_fit
    src = open(os.path.join(REF, "graph_sim_data.py")).read()
    a = src.index("x_data = [")
    b = src.index("#Intended curve for fitting")
    ns = {"np": np}
    exec(compile(src[a:b], "<graph-hist-arrays>", "exec"), ns)
    x, y = np.asarray(ns["x_data"], dtype=np.float64), np.asarray(ns["y_data"], dtype=np.float64)
    assert x.shape == y.shape == (200,)
    popt, _ = curve_fit(lambda t, p, q: p * np.exp(q * np.array(t)), x, y, p0=[14.0, -11.0], maxfev=25000)
    width = x[1] - x[0]
    n_paths = int(round(1.0 / (y[y > 0].min() * width)))
    np.savez_compressed(os.path.join(OUT, "graph_hist.npz"), x=x, density=y, fit_a=popt[0], fit_b=popt[1], n_paths=n_paths)
    print("graph_hist.npz: fit a=%g b=%g -> decay length %.2f nm, %d paths" % (popt[0], popt[1], -1e9 / popt[1], n_paths))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="all")
    a = ap.parse_args()
    os.makedirs(OUT, exist_ok=True)
    if a.only in ("all", "consts"):
        gen_consts()
    if a.only in ("all", "func"):
        gen_func()
    if a.only in ("all", "cube"):
        gen_cube("a", K=6000, sigma_mult=4, steps=40, snaps=[0, 20, 39])
        gen_cube("dense", K=2500, sigma_mult=36, steps=25, snaps=[0, 10, 24])
    if a.only in ("all", "pore"):
        gen_pore("a", K=1500, sigma_mult=100, slice_=1, steps=40, snaps=[0, 1, 5, 20, 39])
    if a.only in ("all", "temp"):
        gen_temp("a", K=2000, sigma_mult=100, slice_=1, steps=30, snaps=[0, 1, 10, 29])
    # the reference's OWN parameters (minutes of run time: not part of "all")
    if a.only in ("all", "graph_hist"):
        gen_graph_hist()
    if a.only == "edge":
        gen_edge()
    if a.only == "clusters":
        gen_clusters()
    if a.only == "resolve":
        gen_resolve()
    if a.only == "temp_edge":
        gen_temp_edge()
    if a.only == "cube_natural":
        gen_cube_natural()
    if a.only == "pore_natural":
        gen_pore_natural()


if __name__ == "__main__":
    main()
