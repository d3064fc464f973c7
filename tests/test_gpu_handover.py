"""The ordered workgroup's hand-over (k_resolve<GEOM, 0>, -m gpu).

When the wide cluster kernel leaves nothing to do, or there were no candidates at all, the ordered workgroup only hands
the sweep's counters over and ends at its first barrier; otherwise its body runs.  A run that alternates the three kinds
of sweep must equal the oracle bit for bit at every step, still report the sweep counters, and the host's lagging copy
of the candidate count must still switch the launch plan.
"""
import re

import numpy as np
import pytest

from argon_monte_carlo_amd import ic as IC
from argon_monte_carlo_amd import params as PR

pytestmark = pytest.mark.gpu

SF = ["x", "y", "z", "vx", "vy", "vz", "d", "dx", "dy", "dz"]
COUNTERS = ("n_pp", "n_wall", "n_oob_walls", "n_oob_pp", "n_paths", "n_fp_errors")


def assert_state_equal(dev, orc, ctx=""):
    for k in SF:
        assert np.array_equal(dev[k], orc[k]), (ctx, k, np.flatnonzero(dev[k] != orc[k])[:5])
    assert np.array_equal(dev["flag"].astype(bool), orc["flag"].astype(bool)), (ctx, "flag")


def _sparse(p, n, vel):
    """Every particle on a lattice point, spacings 2.5 (raised cross-section) to 10 times the collision range, moving a
    thousandth of the usual distance per step: a sweep without candidates."""
    vel = np.asarray(vel) * 1e-3
    m = int(np.ceil(n ** (1.0 / 3.0)))
    idx = np.arange(n)
    ijk = np.stack([idx % m, (idx // m) % m, idx // (m * m)]).astype(np.float64)
    return ((ijk[0] + 0.5) * (p.cube_x / m), (ijk[1] + 0.5) * (p.cube_y / m), (ijk[2] + 0.5) * (p.cube_z / m),
            vel[0], vel[1], vel[2])


def _blobs(p, base, rng):
    """Eight blobs of 20 particles (more than the wide kernel takes in one component) in the usual gas."""
    x, y, z = (np.array(a, dtype=np.float64, copy=True) for a in base[:3])
    cr = p.collision_range
    ext = np.array([p.cube_x, p.cube_y, p.cube_z])
    for b in range(8):
        c = (0.1 + 0.8 * rng.random(3)) * ext
        sel = np.arange(b * 20, (b + 1) * 20)
        off = (rng.random((3, 20)) - 0.5) * 3.0 * cr
        x[sel], y[sel], z[sel] = c[0] + off[0], c[1] + off[1], c[2] + off[2]
    return (x, y, z, base[3], base[4], base[5])


def _debug_lines(eng, capfd):
    """The AMC_DEBUG_RESOLVE figures the library prints when its kernel times are read."""
    capfd.readouterr()
    eng.kernel_times()
    return capfd.readouterr().err


def test_handover_over_idle_empty_and_working_sweeps_vs_oracle(monkeypatch, capfd):
    """Sweeps with no candidates (a lattice), idle sweeps (the ordinary gas: every cluster done by the wide kernel) and
    sweeps the ordered workgroup works on (blobs beyond the wide kernel's component size, and a raised cross-section)
    alternate in one context; state and counters equal the oracle's at every step, and n_candidates / n_clusters /
    n_rounds are reported for the sweeps that had candidates.  The resolve's debug counters show that both the idle
    hand-over and the ordered body ran."""
    from argon_monte_carlo_amd.engine import Engine
    from oracle import oracle as O

    monkeypatch.setenv("AMC_DEBUG_RESOLVE", "1")        # (read at context creation)
    n = 20_000
    rng = np.random.default_rng(7)
    seen_idle = seen_body = 0
    for sigma_mult in (1.0, 16.0):
        p, c = PR.cube_params_for_n(n, sigma=3.6e-19 * sigma_mult)
        p.detect_mode = 1
        p.reserved1 = 1
        init = IC.cube_ic(p, c, seed=127)
        vel = np.array([init[3], init[4], init[5]])
        eng = Engine(p)
        orc = O.Oracle(p, mode="mul", path_capacity=1 << 22)
        kinds = ["usual", "empty", "usual", "blobs", "empty", "blobs", "usual", "usual", "empty", "blobs", "usual"]
        tot = {"n_candidates": 0, "n_clusters": 0, "n_rounds": 0, "n_pp": 0}
        for s, kind in enumerate(kinds):
            if kind != "usual" or s == 0 or kinds[s - 1] != "usual":     # (a "usual" step right after one goes on from it)
                st0 = init if kind == "usual" else (_sparse(p, n, vel) if kind == "empty" else _blobs(p, init, rng))
                eng.upload(*st0)
                orc.upload(*st0)
            st = eng.timestep(c["dt"])
            rc, so = orc.timestep(c["dt"])
            assert rc == 0
            for k in COUNTERS:
                assert st[k] == so[k], (sigma_mult, s, kind, k, st, so)
            assert_state_equal(eng.download(), orc.state(), ("handover", sigma_mult, s, kind))
            if kind == "empty":
                assert st["n_pp"] == 0 and st["n_candidates"] == 0 and st["n_rounds"] == 0, (s, st)
            else:
                assert st["n_candidates"] > 0 and 0 < st["n_clusters"] <= st["n_candidates"], (s, kind, st)
                assert st["n_rounds"] >= 1, (s, kind, st)
            for k in tot:
                tot[k] += st[k]
        assert tot["n_pp"] > 0 and tot["n_candidates"] >= tot["n_pp"], tot
        # launches of the ordered workgroup with candidates, and how many of them only handed the counters over
        m = re.search(r"launches (\d+) \(idle hand-over only (\d+)\)", _debug_lines(eng, capfd))
        assert m, "no AMC_DEBUG_RESOLVE figures"
        launches, idle = int(m.group(1)), int(m.group(2))
        assert launches == 8 and idle <= launches, (sigma_mult, launches, idle)
        seen_idle += idle
        seen_body += launches - idle
        eng.close()
    assert seen_idle > 0 and seen_body > 0, (seen_idle, seen_body)


def test_host_copy_of_the_candidate_count_follows_every_sweep(monkeypatch, capfd):
    """The launch plan (candidates per wave of the wide kernel, extra commit blocks of the streaming pass) is chosen from a
    host-mapped copy of the last sweep's candidate count.  The commit writes it; after every step it holds exactly the
    candidate count that step reported, for small and large sweeps alike."""
    from argon_monte_carlo_amd.engine import Engine
    from oracle import oracle as O

    monkeypatch.setenv("AMC_DEBUG_RESOLVE", "1")
    for n in (20_000, 400_000):
        p, c = PR.cube_params_for_n(n)
        p.reserved1 = 1
        init = IC.cube_ic(p, c, seed=127)
        eng = Engine(p)
        orc = O.Oracle(p, mode="mul", path_capacity=1 << 20)
        eng.upload(*init)
        orc.upload(*init)
        for s in range(4):
            st = eng.timestep(c["dt"])
            rc, so = orc.timestep(c["dt"])
            assert rc == 0
            for k in COUNTERS:
                assert st[k] == so[k], (n, s, k, st, so)
            m = re.search(r"\[amc host candidate count\] (-?\d+)", _debug_lines(eng, capfd))
            assert m, "no AMC_DEBUG_RESOLVE figures"
            assert st["n_candidates"] > 0 and int(m.group(1)) == st["n_candidates"], (n, s, m.group(0), st)
        assert_state_equal(eng.download(), orc.state(), ("host count", n))
        eng.close()
