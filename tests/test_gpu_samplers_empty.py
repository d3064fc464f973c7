"""GPU (-m gpu): every sampler of the particle state on an EMPTY system and on a system of ONE particle, cube and pore.

The host-side scenarios of tests/test_host_sanitized.py found that the pair sampler launched its filing and scatter kernels with
a grid of zero workgroups when n = 0 (amc_pair.hip, pair_launches): every sampled step of an empty system then failed with an
invalid launch configuration.  Here the seven samplers run together on every = 2 over one timestep() and run(5): every call
returns, the totals and counters are those of the exact mirrors (tests/*_ref.py) fed a twin context's downloads — all zero at
n = 0, the one particle's values at n = 1 — and n_samples follows the cadence (the steps 2, 4 and 6)."""
import numpy as np
import pytest

from argon_monte_carlo_amd import params as PR
from tests import together_states as TS
from tests import test_gpu_samplers_together as TG

pytestmark = pytest.mark.gpu

STEPS = 6
EVERY2 = {name: (2, 0) for name in TG.NAMES}
DUE = [2, 4, 6]


def _system(geom, n):
    """(params, dt, state): the reference's cube / pore; the one particle flies at a wall it reaches within the six steps"""
    if geom == "cube":
        p, c = PR.cube_params(n=n)
        dt = c["dt"]
        pos, vel = (50e-9, 40e-9, p.cube_z - 4e-9), (120.0, -80.0, 450.0)
    else:
        p, c = PR.pore_params(n=n)
        dt = TG.PORE_DT_SCALE * c["dt"]
        pos, vel = (3e-9, -2e-9, 6e-9), (90.0, 60.0, -450.0)
    state = [np.full(n, v) for v in pos + vel]
    return p, dt, state


def _step_all(engine, dt):
    """one timestep() and run(5): the six steps, their summed counters"""
    stats = [engine.timestep(dt), engine.run(dt, STEPS - 1)]
    return {k: sum(s[k] for s in stats) for k in TG.COUNTERS}


@pytest.mark.parametrize("n", [0, 1])
@pytest.mark.parametrize("geom", ["cube", "pore"])
def test_all_samplers_on_an_empty_and_a_one_particle_system(geom, n):
    from argon_monte_carlo_amd.engine import Engine
    assert [s for s in range(1, STEPS + 1) if TS.due(2, 0, s)] == DUE
    p, dt, state = _system(geom, n)
    # the twin without a sampler, one timestep() at a time
    twin = Engine(p)
    twin.upload(*state)
    states, records, per_step = [], [], []
    for _ in range(STEPS):
        per_step.append(twin.timestep(dt))
        records.append(twin.drain_paths(sort=False))
        states.append(twin.download())
    twin.close()
    want_stats = {k: sum(s[k] for s in per_step) for k in TG.COUNTERS}
    if n == 1:      # (the particle met its wall and came back: its samples are not all alike)
        assert states[-1]["vz"][0] == -state[5][0] and want_stats["n_pp"] == 0, (states[-1]["vz"], want_stats)
    key = "%s-n%d" % (geom, n)
    TG._TRACE[key] = dict(states=states, records=records)

    e = Engine(p)
    e.upload(*state)
    grids = TG._grids(geom, p)
    TG._configure(e, grids, mix=EVERY2, mfp=False)
    got_stats = _step_all(e, dt)
    assert got_stats == want_stats, (got_stats, want_stats)
    for name in TG.NAMES:
        got = TG._read(e, name)
        assert got["counters"][TG.N_SAMPLES.get(name, 0)] == len(DUE), (name, got["counters"])
        want = TG._mirror(key, name, grids[name], DUE)
        TG._same(got, want, name)
        if n == 0:
            assert not got["totals"].any() and all(v.size == 0 for k, v in got.items() if k in ("origin", "state", "entry")), name
        else:
            assert want["totals"].any(), name
    got = TG._read(e, "free_paths")
    assert got["counters"][2] == STEPS, got["counters"]
    TG._same(got, TG._mirror(key, "free_paths", grids["free_paths"], list(range(1, STEPS + 1))), "free_paths")
    if n == 0:
        assert not got["totals"].any() and not got["hist"].any() and tuple(int(v) for v in got["counters"][:2]) == (0, 0)
    end = e.download()
    for k in TG.KEYS:
        assert end[k].tobytes() == states[-1][k].tobytes(), k
    e.close()
