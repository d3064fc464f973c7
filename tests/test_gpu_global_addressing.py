"""GPU (-m gpu): the resolve kernels after their memory accesses were typed as global (amc_device.h "address spaces",
DESIGN.md 7 round 16).  The change keeps every memory operation, its scope and its order — only the instruction encoding
and the waits the compiler derives from it differ — so the bar is the oracle (`mul`) bit for bit, in state, counters and
completed-path records, once per instantiation the change touches:

  k_clusters_wide<cube>, <pore>     every branch the crafted catalogue proves (tests/cluster_states.py: pair, chain of two,
                                    pull-in with continuation, 4-11 members by the wave, more than 11 on lane 0) and the
                                    hand-over to the ordered workgroup, in the default launch and with AMC_CW_BLOCKS=4
                                    (many clusters in one wave: skip_own, interleaved work items)
  k_resolve<cube, 0>, <pore, 0>     AMC_ORDERED_ALWAYS=1: the ordered workgroup in every sweep of amc_run
  k_resolve<cell, 2>                one single cell through amc_pairwise_cell
  the on-demand plan                amc_run of 8 steps over a hand-over state: the stall word, the rewind, and the commit
                                    that rides along in k_stream

What the instructions are is tests/test_isa_addressing.py's business (no GPU needed)."""
import numpy as np
import pytest

from argon_monte_carlo_amd import params as PR
from tests import cluster_states as CS
from tests.test_gpu_cluster_limits import oracles  # noqa: F401  (fixture: one oracle run per state and sequence of calls)
from tests.test_gpu_edges import Engine, O, _pair, _steps  # noqa: F401  (Engine, O: fixtures)

pytestmark = pytest.mark.gpu

# one state with everything the wide kernel finishes alone, then one per way of leaving work to the ordered workgroup that
# goes through different converted stores: a component it does not take (`changed`), a fifth pull (slot taken by the
# probe, plain merge edge), a third hit on a pair (counter-allocated history entries), a conflict found in the overlay
WIDE_STATES = ("within", "chain_17", "pulls_5", "pair_pull2", "conflict_overlay")
ON_DEMAND_STEPS = 8


@pytest.mark.parametrize("which", WIDE_STATES)
@pytest.mark.parametrize("blocks", [None, 4])
@pytest.mark.parametrize("kind", CS.KINDS)
def test_wide_kernel_equals_the_oracle(Engine, oracles, monkeypatch, kind, blocks, which):
    if blocks:
        monkeypatch.setenv("AMC_CW_BLOCKS", str(blocks))        # (read at context creation)
    s = CS.catalogue(kind, "identity", which)
    ctx = (kind, blocks, which)
    OT = oracles(kind, "identity", which, "1, 1, 2")
    eng, orc = _pair(Engine, OT, s, detect_mode=1)
    if blocks:
        # a warm-up sweep of the same state: the host's lagging candidate count then packs the candidates into the waves
        eng.timestep(s.dt)
        a = s.arrays()
        eng.upload(*a[:10], flag=a[10])
        eng.drain_paths()
    _steps(eng, orc, s, (1, 1, 2), ctx)
    eng.close()
    OT.done()


@pytest.mark.parametrize("which", ("within", "chain_17"))
@pytest.mark.parametrize("kind", CS.KINDS)
def test_ordered_workgroup_in_every_sweep(Engine, oracles, monkeypatch, kind, which):
    monkeypatch.setenv("AMC_ORDERED_ALWAYS", "1")
    s = CS.catalogue(kind, "identity", which)
    OT = oracles(kind, "identity", which, "run")
    eng, orc = _pair(Engine, OT, s, detect_mode=1)
    _steps(eng, orc, s, (ON_DEMAND_STEPS,), (kind, which, "ordered always"))
    assert eng.overlap_stats()["on_demand_steps"] == 0
    eng.close()
    OT.done()


@pytest.mark.parametrize("which", ("chain_17", "conflict_overlay"))
@pytest.mark.parametrize("kind", CS.KINDS)
def test_on_demand_run_over_a_hand_over(Engine, oracles, monkeypatch, kind, which):
    monkeypatch.delenv("AMC_ORDERED_ALWAYS", raising=False)
    s = CS.catalogue(kind, "identity", which)
    OT = oracles(kind, "identity", which, "run")
    eng, orc = _pair(Engine, OT, s, detect_mode=1)
    _steps(eng, orc, s, (ON_DEMAND_STEPS,), (kind, which, "on demand"))
    od = eng.overlap_stats()
    assert od["on_demand_steps"] >= ON_DEMAND_STEPS and od["stalls"] > 0, od     # the sticky word was raised and answered
    eng.close()
    OT.done()


def _cell_state(p, m=3):
    """m^3 particles on a lattice of 0.7 collision ranges inside one cell, every one with a speed and direction of its
    own: neighbours overlap, so the in-place i > j loop runs through long chains; every second one has a path open"""
    cr = p.collision_range
    g = np.arange(m, dtype=np.float64)
    x, y, z = (a.ravel() * 0.7 * cr for a in np.meshgrid(g, g, g, indexing="ij"))
    k = np.arange(m ** 3, dtype=np.float64)
    vx, vy, vz = 100.0 + 7.0 * k, -60.0 + 11.0 * ((k * 5) % 9), 30.0 - 13.0 * ((k * 3) % 7)
    cont, cx, cy, cz = (1.0 + k) * 1e-9, (2.0 + k) * 1e-10, (3.0 + k) * 1e-10, (4.0 + k) * 1e-10
    flag = (np.arange(m ** 3) % 2).astype(np.uint8)
    return [cont, cx, cy, cz, flag, x, y, z, vx, vy, vz]


def test_single_cell_equals_the_oracle(Engine, O):
    p, _ = PR.cell_params(n=27)
    state = _cell_state(p)
    ref, rpaths, rnc, rc = O.pair_cell(p, *state, mode="mul")
    assert rc == 0 and rnc >= 27 and len(rpaths) > 0            # chains, not single pairs; completed paths among them
    args = [np.ascontiguousarray(a, dtype=np.uint8 if q == 4 else np.float64) for q, a in enumerate(state)]
    eng = Engine(p)
    paths, nc = eng.pairwise_cell(*args)
    assert nc == rnc
    for f, a in zip(("cont", "cx", "cy", "cz", "flag", "x", "y", "z", "vx", "vy", "vz"), args):
        assert np.array_equal(a.astype(np.float64), ref[f].astype(np.float64)), f
    assert np.array_equal(paths, rpaths)                        # the same values in the same (reference) order
    eng.close()
