"""GPU (-m gpu): the two forms of the overlay half of the wide cluster kernel's validation (amc_clusters.hip, 4b) — the
DENSE scan of the candidates' history records, taken by sweeps of up to AMC_CW_DENSE_MAX candidates that fit one pass of
the launch, and the per-cell overlay LISTS above that — on the crafted clusters of tests/cluster_states.py.  Bar: that
module's — bit for bit equal to the oracle (`mul`) after every call, in state, counters and completed-path records.

Which form a sweep took is read from the debug instantiation's figures (AMC_DEBUG_RESOLVE): `dense scans` counts the timed
waves that validated by the scan, `dense sweeps linked` the non-idle ordered-workgroup passes that linked the wide kernel's
records into the overlay lists themselves.

Not here: a conflict_overlay state in which one of the two conflicting pairs is itself handed over — the catalogue offers
none (its hand-over states put an ordinary pair beside the cluster, too far away to conflict with it)."""
import re

import pytest

from tests import cluster_states as CS
from tests.test_gpu_edges import Engine, O, _pair, _steps, assert_state_equal  # noqa: F401  (Engine, O: fixtures)

pytestmark = pytest.mark.gpu

DENSE = "512"               # AMC_CW_DENSE_MAX of the dense sides: one candidate per wave of the default launch, above every count here
ON_DEMAND_STEPS = 8         # as tests/test_gpu_cluster_limits.py: amc_run launches the ordered workgroup on demand from 8 steps on


def _figures(eng, capfd):
    """(timed waves that took the dense scan, ordered-workgroup launches, idle ones, dense sweeps it linked)"""
    capfd.readouterr()
    eng.kernel_times()
    err = capfd.readouterr().err
    md = re.search(r"dense scans (\d+)", err)
    ml = re.search(r"launches (\d+) \(idle hand-over only (\d+)\)", err)
    mk = re.search(r"dense sweeps linked (\d+)", err)
    assert md and ml and mk, err
    return int(md.group(1)), int(ml.group(1)), int(ml.group(2)), int(mk.group(1))


def _warm(eng, s):
    """one sweep of the same state, then the state again: the host's lagging candidate count now sizes the wide kernel's
    pass (with AMC_CW_BLOCKS=4, up to 64 candidates per wave) — and a dense sweep needs one pass to hold it"""
    eng.timestep(s.dt)
    a = s.arrays()
    eng.upload(*a[:10], flag=a[10])
    eng.drain_paths()


# ---------------------------------------------------------------------------------------------------------------- 1. lists
@pytest.mark.parametrize("which", ["within", "conflict_overlay", "conflict_grid"])
@pytest.mark.parametrize("blocks", [0, 4])
@pytest.mark.parametrize("kind", CS.KINDS)
def test_list_form_is_still_reachable_at_small_sizes(Engine, O, monkeypatch, capfd, kind, blocks, which):
    """AMC_CW_DENSE_MAX=0: every sweep validates through the overlay lists, as before"""
    monkeypatch.setenv("AMC_CW_DENSE_MAX", "0")
    monkeypatch.setenv("AMC_DEBUG_RESOLVE", "1")
    if blocks:
        monkeypatch.setenv("AMC_CW_BLOCKS", str(blocks))
    for perm in CS.PERMS:
        s = CS.catalogue(kind, perm, which)
        ctx = ("lists", kind, perm, which, blocks)
        eng, orc = _pair(Engine, O, s, detect_mode=1)
        if blocks:
            _warm(eng, s)
        _steps(eng, orc, s, (1, 1, 3), ctx)
        dense, _, _, linked = _figures(eng, capfd)
        assert dense == 0 and linked == 0, (ctx, dense, linked)
        eng.close()


# ---------------------------------------------------------------------------------------------------------------- 2. threshold
@pytest.mark.parametrize("kind", CS.KINDS)
def test_the_two_sides_of_the_threshold(Engine, O, monkeypatch, capfd, kind):
    """C candidates in the first sweep of `within`: dense at AMC_CW_DENSE_MAX = C, lists at C - 1; both equal the oracle and
    each other"""
    monkeypatch.setenv("AMC_DEBUG_RESOLVE", "1")
    s0 = CS.catalogue(kind, "identity", "within")
    C = len(CS.structure(s0)["pairs"])
    assert 1 < C <= 512, C                      # (512 waves, one candidate each: one pass holds them)
    states = {}
    for side, dense_max in (("dense", C), ("lists", C - 1)):
        monkeypatch.setenv("AMC_CW_DENSE_MAX", str(dense_max))
        s = CS.catalogue(kind, "identity", "within")
        ctx = ("threshold", kind, side, C)
        eng, orc = _pair(Engine, O, s, detect_mode=1)
        st = eng.timestep(s.dt)
        rc, so = orc.timestep(s.dt)
        assert rc == 0 and st["n_pp"] == so["n_pp"] and st["n_candidates"] == C, (ctx, st, so)
        assert_state_equal(eng.download(), orc.state(), ctx)
        dense = _figures(eng, capfd)[0]
        print(ctx, "timed waves that took the dense scan:", dense)
        assert (dense > 0) == (side == "dense"), (ctx, dense)
        _steps(eng, orc, s, (1, 3), ctx)
        states[side] = eng.download()
        eng.close()
    assert_state_equal(states["dense"], states["lists"], ("threshold", kind))


# ---------------------------------------------------------------------------------------------------------------- 3. one wave
@pytest.mark.parametrize("which", ["conflict_overlay", "items_fit"])
@pytest.mark.parametrize("kind", CS.KINDS)
def test_dense_with_many_clusters_per_wave(Engine, O, monkeypatch, capfd, kind, which):
    """AMC_CW_BLOCKS=4 after a warm-up sweep: up to 64 clusters in one wave, ONE read of the candidates' records tested
    against all of the wave's items.  conflict_overlay holds both pinned index orders of the two conflicting pairs: the merge
    edge must arrive (the ordered workgroup's pass is not idle, and it links the dense sweep's records itself); the 40
    two-hit clusters of items_fit conflict with nobody (an idle pass)."""
    monkeypatch.setenv("AMC_CW_BLOCKS", "4")
    monkeypatch.setenv("AMC_CW_DENSE_MAX", DENSE)
    monkeypatch.setenv("AMC_DEBUG_RESOLVE", "1")
    for perm in CS.PERMS:
        s = CS.catalogue(kind, perm, which)
        ctx = ("one wave", kind, perm, which)
        eng, orc = _pair(Engine, O, s, detect_mode=1)
        _warm(eng, s)
        d0, l0, i0, k0 = _figures(eng, capfd)
        _steps(eng, orc, s, (1,), ctx)
        d1, l1, i1, k1 = _figures(eng, capfd)
        print(ctx, "dense scans", d0, d1, "launches", l0, l1, "idle", i0, i1, "linked", k0, k1)
        assert d1 > d0 and l1 - l0 == 1, (ctx, d0, d1, l0, l1)
        if which == "conflict_overlay":
            assert i1 - i0 == 0 and k1 - k0 == 1, (ctx, i0, i1, k0, k1)
        else:
            assert i1 - i0 == 1 and k1 == k0, (ctx, i0, i1, k0, k1)
        _steps(eng, orc, s, (1, 2), ctx)
        eng.close()


# ---------------------------------------------------------------------------------------------------------------- 4. stale
@pytest.mark.parametrize("which", ["conflict_overlay", "within"])
@pytest.mark.parametrize("kind", CS.KINDS)
def test_stale_records_of_the_last_sweep_count_for_nothing(Engine, O, monkeypatch, kind, which):
    """ON_DEMAND_STEPS steps of amc_run (the ordered workgroup on demand): candidate indices are reused from sweep to sweep
    while the clusters stay at their sites, so entry 4k still holds the last sweep's record of slot 2k when the new owner
    of slot 2k initialises it with round 1 — the detect kernel has cleared its tag.  Equal to the oracle, and no more
    launches of the ordered workgroup than the list form needs for the same run.  The threshold is set for both sides, whatever
    the default: 512 is one candidate per wave of the default launch and above every candidate count of these states, so
    every sweep of that side is dense (the debug figures cannot say so here: with AMC_DEBUG_RESOLVE amc_run launches the
    ordered workgroup in every sweep)."""
    monkeypatch.delenv("AMC_DEBUG_RESOLVE", raising=False)
    launches = {}
    for side, dense_max in (("dense", DENSE), ("lists", "0")):
        monkeypatch.setenv("AMC_CW_DENSE_MAX", dense_max)
        s = CS.catalogue(kind, "identity", which)
        ctx = ("stale", kind, which, side)
        eng, orc = _pair(Engine, O, s, detect_mode=1)
        _steps(eng, orc, s, (ON_DEMAND_STEPS,), ctx)
        od = eng.overlap_stats()
        assert od["on_demand_steps"] >= ON_DEMAND_STEPS, (ctx, od)
        launches[side] = od["ordered_launches"]
        eng.close()
    print(kind, which, launches)
    assert launches["dense"] <= launches["lists"], (kind, which, launches)


# ---------------------------------------------------------------------------------------------------------------- 5. ordered
@pytest.mark.parametrize("which", ["chain_17", "pair_pull2"])
@pytest.mark.parametrize("kind", CS.KINDS)
def test_dense_sweep_with_a_working_ordered_workgroup(Engine, O, monkeypatch, capfd, kind, which):
    """a cluster that is handed over beside its company pair, in a dense sweep: the ordered workgroup validates through the
    overlay lists, which the wide kernel no longer fills — it links the company pair's record itself"""
    monkeypatch.setenv("AMC_CW_DENSE_MAX", DENSE)
    monkeypatch.setenv("AMC_DEBUG_RESOLVE", "1")
    for perm in CS.PERMS:
        s = CS.catalogue(kind, perm, which)
        ctx = ("ordered", kind, perm, which)
        eng, orc = _pair(Engine, O, s, detect_mode=1)
        _steps(eng, orc, s, (1,), ctx)
        dense, launches, idle, linked = _figures(eng, capfd)
        print(ctx, "dense scans", dense, "launches", launches, "idle", idle, "linked", linked)
        assert dense > 0 and launches == 1 and idle == 0 and linked == 1, (ctx, dense, launches, idle, linked)
        _steps(eng, orc, s, (1, 3), ctx)
        eng.close()
