"""The first round trips of the step's kernels ("first trips").  k_clusters_wide asks for its first candidate,
the candidate count and the stall word through pointers it takes from the kernarg segment, between the loads and the
stores of the copy of its argument block to LDS.  Only where loads are issued differs from a plain entry, so every run
here must equal the CPU oracle bit for bit — state, counters, completed paths, histograms — at the inputs where a load on
the wrong side of a test would show: the speculative first candidate at its edges and, for the streaming pass's slot
word and stall test, slots of both kinds and stalled steps."""
import numpy as np
import pytest

from argon_monte_carlo_amd import ic as IC
from argon_monte_carlo_amd import params as PR
from tests.test_gpu_ordered_on_demand import (assert_histograms_equal_oracle, bench_like, check_both_modes, dense_blob,
                                              oracle_chunks, run_chunks, stress)
from tests.test_gpu_parity import assert_state_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def Engine():
    from argon_monte_carlo_amd.engine import Engine as E
    return E


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def sorted_rows(a):
    return a[np.lexsort(a.T[::-1])]


def check_run(Engine, O, p, dt, init, steps, ctx):
    """One amc_run of `steps` steps against the oracle: statistics, state, completed paths, histograms.  Returns the
    engine's statistics and overlap_stats."""
    sums, ref_state, ref_paths = oracle_chunks(O, p, dt, init, [steps])
    stats, state, hist, paths, ov = run_chunks(Engine, p, dt, init, [steps])
    for k in sums[0]:
        assert stats[0][k] == sums[0][k], (ctx, k, stats[0], sums[0])
    assert_state_equal(state, ref_state, ctx)
    assert paths.shape == ref_paths.shape, ctx
    assert np.array_equal(sorted_rows(paths), sorted_rows(ref_paths)), ctx
    assert_histograms_equal_oracle(p, hist, ref_paths, ctx)
    return stats[0], ov


# ---- k_stream: slots whose sweep moved the particle, and slots whose sweep did not ------------------------------------------
TWIN_N, TWIN_STEPS, TWIN_SEED = 3000, 36, 10


def cube_with_comoving_twins():
    """A dense cube (the stress inputs of test_gpu_parity at N = 3,000: some forty collisions in every step) plus one designed
    pair: particles 0 and 1 overlap and move with the SAME velocity.  The pair is a candidate in every sweep, its contact
    solve has no solution (zero relative velocity: counted in n_fp_errors, nothing moved — Temp:340-342 semantics,
    reserved1), so both hold a slot with `moved` clear in every sweep, next to the slots of the particles that did collide.
    The seed is one for which the oracle shows that nobody else touches the two in TWIN_STEPS steps."""
    p, c = PR.cube_params_for_n(TWIN_N, sigma=3.6e-19 * 16.0)
    init = [np.array(a, dtype=np.float64) for a in IC.cube_ic(p, c, seed=TWIN_SEED)]
    p.detect_mode = 1
    p.reserved1 = 1
    mid = (0.5 * p.cube_x, 0.5 * p.cube_y, 0.5 * p.cube_z)
    for axis in range(3):
        init[axis][0] = mid[axis]
        init[axis][1] = mid[axis] + (0.4 * p.collision_range if axis == 0 else 0.0)
        init[3 + axis][0] = init[3 + axis][1] = 1.0 + axis            # (m/s: they stay in the middle of the cube)
    return p, c["dt"], tuple(init)


def test_slots_with_and_without_a_moved_particle(Engine, O):
    p, dt, init = cube_with_comoving_twins()
    # the precondition, from the statistics of every single step: a collision (a slot with `moved` set) and the skipped
    # contact solve of the twins (two slots with it clear) in EVERY sweep — the oracle's steps; the run below must show
    # the same sums
    orc = O.Oracle(p, mode="mul")
    orc.upload(*init)
    for s in range(TWIN_STEPS):
        rc, st = orc.timestep(dt)
        assert rc == 0 and st["n_pp"] >= 1 and st["n_fp_errors"] >= 1, (s, st)
    ref = orc.state()
    for k, v in (("vx", 1.0), ("vy", 2.0), ("vz", 3.0)):
        assert ref[k][0] == v and ref[k][1] == v, k                  # never moved by anybody: their slots were clear throughout
    stats, ov = check_run(Engine, O, p, dt, init, TWIN_STEPS, "twins")
    assert stats["n_fp_errors"] >= TWIN_STEPS and stats["n_pp"] >= TWIN_STEPS, stats
    assert ov["on_demand_steps"] >= TWIN_STEPS, ov                   # (the headline's plan ran)
    # the same through single steps, whose statistics are the device's own per sweep (results still picked up by the next
    # step's streaming pass)
    eng = Engine(p)
    eng.upload(*init)
    for s in range(12):
        st = eng.timestep(dt)
        assert st["n_pp"] >= 1 and st["n_fp_errors"] >= 1 and st["n_candidates"] >= 2, (s, st)
    eng.close()


# ---- k_stream: a stalled step leaves nothing behind ----------------------------------------------------------------------------
def test_stalled_steps_leave_nothing_behind(Engine, O, monkeypatch):
    """The dense blob: most sweeps need the ordered workgroup, so the steps enqueued behind them are stalled, do nothing and are
    enqueued again.  A store of the streaming pass in front of its stall test (slot_of[p] = -1 above all) would lose a
    sweep's result: the run would differ from the one with the ordered workgroup in every sweep, and from the oracle."""
    p, dt, init = dense_blob()
    od, al = check_both_modes(Engine, O, monkeypatch, p, dt, init, [16], "stalled")
    assert od["stalls"] > 0 and od["on_demand_steps"] > 16, od
    assert al["stalls"] == 0, al


# ---- k_clusters_wide: the speculative first candidate at its edges -----------------------------------------------------------
def test_sweeps_without_a_candidate(Engine, O):
    """Dilute, N = 1,000, 512 waves of one candidate each: no sweep has more than a handful of candidates, so the first
    candidate that all but a few waves asked for lies beyond the candidate count, and in a sweep with none (asserted: the
    device's own count per step) every wave's does — stale memory of an earlier sweep."""
    p, dt, init = bench_like("cube", 1000)
    steps = 24
    eng = Engine(p)
    eng.upload(*init)
    per_step = [eng.timestep(dt)["n_candidates"] for _ in range(steps)]
    eng.close()
    assert min(per_step) == 0 and 1 <= max(per_step) <= 64, per_step
    stats, ov = check_run(Engine, O, p, dt, init, steps, "dilute")
    assert ov["on_demand_steps"] >= steps, ov


def test_four_waves_and_several_hundred_candidates(Engine, O, monkeypatch):
    """AMC_CW_BLOCKS=4: 64 candidates per wave and pass, and more than 4 x 64 candidates in EVERY sweep (asserted: the
    device's own count per step), so every wave makes several passes — in all but the first its candidates are not the one it
    asked for at its entry, and in the last pass the lanes of most waves lie beyond the candidate count."""
    monkeypatch.setenv("AMC_CW_BLOCKS", "4")
    p, dt, init = stress("cube", 30_000, 16.0)
    steps = 10
    eng = Engine(p)
    eng.upload(*init)
    per_step = [eng.timestep(dt)["n_candidates"] for _ in range(steps)]
    eng.close()
    assert min(per_step) > 4 * 64, per_step
    stats, ov = check_run(Engine, O, p, dt, init, steps, "four waves")
    assert stats["n_candidates"] == sum(per_step), (stats, per_step)


ONE_N, ONE_STEPS, ONE_SEED = 120, 40, 7


def close_pairs(st, r2):
    x, y, z = st["x"], st["y"], st["z"]
    d2 = (x[:, None] - x[None, :]) ** 2 + (y[:, None] - y[None, :]) ** 2 + (z[:, None] - z[None, :]) ** 2
    return int((d2[np.triu_indices(len(x), 1)] < r2).sum())


def test_candidate_capacity_of_one(Engine, O):
    """max_candidates = 1, the smallest capacity the API takes: `k_first < max_cand` holds for one lane of one wave only.  The
    seed is one whose sweeps never hold two candidates and hold one eleven times: counted here on the oracle's state in
    front of every sweep, within 2 % more than the collision range so that no rounding of the detector decides it."""
    p, c = PR.cube_params_for_n(ONE_N)
    init = IC.cube_ic(p, c, seed=ONE_SEED)
    p.reserved1 = 1
    p.max_candidates = 1
    dt = c["dt"]
    orc = O.Oracle(p, mode="mul")
    orc.upload(*init)
    per_step = []
    for _ in range(ONE_STEPS):
        orc.drift(dt)
        orc.cube_walls()
        st = orc.state()
        per_step.append(close_pairs(st, p.collision_range ** 2))
        assert close_pairs(st, (1.02 * p.collision_range) ** 2) == per_step[-1], per_step
        orc.sweep()
    assert max(per_step) == 1 and sum(per_step) >= 2, per_step
    stats, _ = check_run(Engine, O, p, dt, init, ONE_STEPS, "capacity 1")
    assert stats["n_candidates"] == sum(per_step), (stats, per_step)


# ---- the pore: the wide kernel's other instantiation ---------------------------------------------------------------------------
def test_pore_once(Engine, O):
    p, dt, init = stress("pore", 20_000, 30.0)
    stats, ov = check_run(Engine, O, p, dt, init, 20, "pore")
    assert stats["n_pp"] >= 20 and stats["n_candidates"] >= 20, stats     # (the wide kernel had candidates to resolve)
    assert ov["on_demand_steps"] >= 20, ov
