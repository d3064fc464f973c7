"""Scenarios of the sampled free paths' tests (tests/test_mfp_host.py, tests/test_gpu_mfp.py).  Paths complete only for
particles whose full_path_traveled flag is set, and the synthetic initial conditions have it clear: every scenario is the
generator's positions and velocities (seed 11) with dist_* = 0 and all flags = 1.

  A  cube, N = 20,011, natural sigma, 7 steps: p-p paths in every step, no wall paths
  B  pore, N = 20,000, natural sigma, 7 steps: wall and p-p paths, a handful per step
  C  pore, N = 20,000, sigma = 3.6e-17, 2 steps: 3,024 p-p paths in step 1 (two full strides of the sampler's workgroup and a
     tail), 267 of them a second or later path of the same owner in that step
"""
import functools

import numpy as np

from argon_monte_carlo_amd import ic as IC
from argon_monte_carlo_amd import params as PR

SEED = 11
SIGMA_C = 3.6e-17
STEPS = {"A": 7, "B": 7, "C": 2}
# completed paths per step as the CPU oracle ("mul" arithmetic) counts them: (wall, p-p)
ORACLE_COUNTS = {
    "A": [(0, 72), (0, 82), (0, 84), (0, 66), (0, 48), (0, 52), (0, 52)],
    "B": [(0, 4), (2, 0), (7, 4), (9, 0), (13, 2), (16, 0), (11, 2)],
    "C": [(None, 3024), (None, 186)],
}


def scenario_params(name, max_paths=None):
    """(params, consts, kind) of scenario ``name``"""
    if name == "A":
        p, c = PR.cube_params(n=20_011)         # (the reference's own 100 nm cube)
        kind = "cube"
    else:
        p, c = PR.pore_params(n=20_000, sigma=SIGMA_C) if name == "C" else PR.pore_params(n=20_000)
        kind = "pore"
    if max_paths is not None:
        p.max_paths = int(max_paths)
    return p, c, kind


@functools.lru_cache(maxsize=None)
def _ic(name):
    p, c, kind = scenario_params(name)
    return tuple((IC.cube_ic if kind == "cube" else IC.pore_ic)(p, c, SEED))


def initial_state(name):
    """the eleven arrays of ``Simulation.set_state``: positions and velocities of the generator, zero distances, all flags set"""
    x, y, z, vx, vy, vz = [np.array(a, dtype=np.float64) for a in _ic(name)[:6]]
    zero = np.zeros(len(x))
    return [x, y, z, vx, vy, vz, zero, zero.copy(), zero.copy(), zero.copy(), np.ones(len(x), dtype=np.uint8)]


def energised_state(n, seed=SEED):
    p, c = PR.pore_params(n=n, energised=True)
    x, y, z, vx, vy, vz = [np.array(a, dtype=np.float64) for a in IC.pore_ic(p, c, seed)[:6]]
    zero = np.zeros(n)
    return [x, y, z, vx, vy, vz, zero, zero.copy(), zero.copy(), zero.copy(), np.ones(n, dtype=np.uint8)]


@functools.lru_cache(maxsize=None)
def oracle_steps(name):
    """The CPU oracle's run of scenario ``name``: [(records drained after the step, state after the step)] per step."""
    from oracle.oracle import Oracle
    p, c, _ = scenario_params(name)
    o = Oracle(p, "mul")
    s = initial_state(name)
    o.upload(*s[:10], flag=s[10])
    out = []
    for _ in range(STEPS[name]):
        rc, _st = o.timestep(c["dt"])
        assert rc == 0
        out.append((o.drain_paths(), o.state()))
    return out
