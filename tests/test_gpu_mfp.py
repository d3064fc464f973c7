"""GPU (-m gpu): the sampled free paths (include/argonmc_mfp.h) against tests/mfp_ref.py, bit for bit.

The reference is fed what the context itself hands out — after every step the drained path records (keep_records = 1) and the
downloaded state — so every comparison is between the device's binning and the header's rule on the same records.  The
scenarios are tests/mfp_states.py's: A cube, B pore, C pore with a raised cross-section (3,024 paths in one step).  Each test
asserts from its own reference that it has binned something before it compares."""
import numpy as np
import pytest
import torch                # (first: the library then shares torch's HIP runtime — the sharded tests exchange through torch)

from argon_monte_carlo_amd import free_paths as FP
from argon_monte_carlo_amd._abi import AMC_ERR_CAPACITY, AMC_ERR_STATE
from argon_monte_carlo_amd._lib import ArgonMCError
from argon_monte_carlo_amd.sim import Simulation
from tests import mfp_ref as REF
from tests import mfp_states as MS
from tests.sampler_states import ODD_SHARDS

pytestmark = pytest.mark.gpu

KEYS = ("x", "y", "z", "vx", "vy", "vz", "d", "dx", "dy", "dz", "flag")
COUNTERS = ("n_pp", "n_wall", "n_oob_walls", "n_oob_pp", "n_paths", "n_fp_errors")


def make_sim(name, grid="default", keep=True, max_paths=None, state=None, shard=False):
    """scenario ``name`` uploaded into a new context; grid None: no sampler, "default": the geometry's; shard: a ShardEngine
    over the whole index range, which the sharded step's calls can drive as well"""
    p, c, kind = MS.scenario_params(name, max_paths)
    engine = None
    if shard:
        from argon_monte_carlo_amd.engine import ShardEngine
        engine = ShardEngine(p, 0, int(p.n))
    sim = Simulation(kind=kind, params=p, consts=c, engine=engine)
    sim.set_state(*(MS.initial_state(name) if state is None else state))
    if grid is not None:
        sim.enable_free_paths(None if isinstance(grid, str) else grid, keep_records=keep)
    return sim


def grids(name):
    """the grids of test 1: the default, one bin, one at the column limit and, in the pore, a Cartesian one over its bounding box"""
    p, _, kind = MS.scenario_params(name)
    if kind == "cube":
        lo, hi = (0.0, 0.0, 0.0), (p.cube_x, p.cube_y, p.cube_z)
        return {"default": FP.default_grid(p), "one": FP.make_grid("cartesian", (1, 1, 1), lo, hi),
                "limit": FP.make_grid("cartesian", (4, 4, 4), lo, hi, hist_bins=40, hist_hi=2e-7)}
    return {"default": FP.default_grid(p), "one": FP.make_grid("axisymmetric", (1, 1), (0.0, 0.0), (p.R_oa, p.H)),
            "limit": FP.make_grid("axisymmetric", (4, 12), (0.0, 0.0), (p.R_oa, p.H), hist_bins=56, hist_hi=2e-7),
            "box": FP.make_grid("cartesian", (4, 4, 6), (-p.R_oa, -p.R_oa, 0.0), (p.R_oa, p.R_oa, p.H), hist_bins=16)}


def check(engine, ref):
    """totals, histograms and counters of the context equal the reference's, bit for bit"""
    tot, hist, counters = engine.mfp_read()
    assert counters == ref.counters()
    assert np.array_equal(hist, ref.hist)
    assert np.array_equal(tot, ref.words())
    return tot


_TRACE = {}


def stepwise(name, grid="default", steps=None, max_paths=None):
    """A keep-mode context stepped with timestep(collect_paths=False), a state download and a drain after every step:
    (sim, the reference fed those records and states).  The first run of a scenario leaves its trace — per step the records
    and the positions, at the end the state, the histograms and the summed counters — for the tests that run otherwise."""
    sim = make_sim(name, grid, keep=True, max_paths=max_paths)
    ref = REF.Totals(sim.engine.mfp_grid)
    trace, total = [], dict.fromkeys(COUNTERS, 0)
    for _ in range(MS.STEPS[name] if steps is None else steps):
        st = sim.timestep(collect_paths=False)
        for k in COUNTERS:
            total[k] += st[k]
        state = sim.engine.download()
        rec = sim.engine.drain_paths(sort=False)
        ref.add_step(rec, state)
        trace.append((rec, {k: state[k] for k in "xyz"}))
    if name not in _TRACE and steps is None and max_paths is None:
        _TRACE[name] = dict(steps=trace, state=sim.engine.download(), hist=sim.engine.histograms(), counters=total)
    return sim, ref


def trace(name):
    if name not in _TRACE:
        stepwise(name)[0].close()
    return _TRACE[name]


def reference(name, grid, first=0, last=None):
    """the reference on the scenario's trace, steps [first, last)"""
    ref = REF.Totals(grid)
    for rec, st in trace(name)["steps"][first:last]:
        ref.add_step(rec, st)
    return ref


def kinds_per_step(name):
    return [(int((REF.owners_and_kinds(rec)[1] == 0).sum()), int(REF.owners_and_kinds(rec)[1].sum())) for rec, _ in trace(name)["steps"]]


def assert_scenario_has_work(name):
    """the issue's preconditions, from the test's own records"""
    per = kinds_per_step(name)
    if name == "A":
        assert all(pp > 0 for _, pp in per), per
    elif name == "B":
        assert sum(w for w, _ in per) > 0 and sum(pp for _, pp in per) > 0, per
    else:
        owner = REF.owners_and_kinds(trace("C")["steps"][0][0])[0]
        assert len(owner) > 2048 and len(owner) - len(np.unique(owner)) >= 1
    assert per == [(w if w is not None else per[k][0], pp) for k, (w, pp) in enumerate(MS.ORACLE_COUNTS[name])]      # (the CPU oracle's counts)


# ---- 1. totals equal the reference, step by step (and 3: the cube's deferred results) -------------------------------------------
@pytest.mark.parametrize("name,which", [(n, g) for n in "ABC" for g in ("default", "one", "limit")] + [("B", "box"), ("C", "box")])
def test_totals_equal_reference_after_timesteps(name, which):
    """Scenario A is test 3 as well: in the cube a step's sweep leaves its results in the slot arrays (nothing applies them
    before the next step's streaming pass), so the hook's launch bins the colliding owners' positions through slot_of[] —
    the download behind it flushes them, and the reference bins the flushed positions.  No entry point exposes lazy_pending,
    so that it was pending is not asserted here; a launch that ignored the slot arrays would bin the pre-collision
    positions of all the p-p owners and miss the reference wherever one of them crossed a bin edge."""
    g = grids(name)[which]
    sim, ref = stepwise(name, g)
    assert_scenario_has_work(name)
    ref.check()
    tot = check(sim.engine, ref)
    assert ref.n_records > 0 and tot[..., 0].any() and ref.n_steps == MS.STEPS[name]
    if which == "box":
        inside = reference(name, grids(name)["one"])
        assert ref.n_records + ref.n_outside == inside.n_records + inside.n_outside     # every record is binned or counted outside
    f = sim.free_paths()
    assert f["count"][:, 2].sum() == ref.n_records and np.isfinite(f["mean_free_path"][f["count"] > 0]).all()
    assert sim.engine.paths_pending() == 0          # (drained after every step)
    sim.close()


# ---- 2. run(k) equals k timesteps; the sampler is the records' reader and changes nothing else ---------------------------------
@pytest.mark.parametrize("name", ["A", "B", "C"])
@pytest.mark.parametrize("env", [{}, {"AMC_OVERLAP": "1"}, {"AMC_LIST_KEEP": "4"}], ids=["plain", "overlap", "list_keep4"])
def test_run_equals_timesteps_and_leaves_everything_else_alone(name, env, monkeypatch):
    assert_scenario_has_work(name)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    k = MS.STEPS[name]
    sim = make_sim(name, keep=False)
    st = sim.run(k)
    ref = reference(name, sim.engine.mfp_grid)
    check(sim.engine, ref)
    assert sim.engine.paths_pending() == 0 and len(sim.engine.drain_paths()) == 0
    base = make_sim(name, grid=None)
    st0 = base.run(k)
    a, b = sim.engine.download(), base.engine.download()
    for key in KEYS:
        assert np.array_equal(a[key], b[key]), key
        assert np.array_equal(a[key], trace(name)["state"][key]), key
    (ha, na), (hb, nb) = sim.engine.histograms(), base.engine.histograms()
    assert na == nb == trace(name)["hist"][1] and np.array_equal(ha, hb) and np.array_equal(ha, trace(name)["hist"][0])
    assert {c: st[c] for c in COUNTERS} == {c: st0[c] for c in COUNTERS} == trace(name)["counters"]
    assert base.engine.paths_pending() == ref.n_records + ref.n_outside      # (without the sampler the records pile up)
    sim.close()
    base.close()


# ---- 4. range and loss -------------------------------------------------------------------------------------------------------
def test_a_path_out_of_range_is_named_and_stops_the_accumulation_until_reset():
    state = MS.initial_state("A")
    state[6] = np.full(len(state[0]), 1e-4)         # dist_since_collision: every completed path is about 1e-4 m > 2^-16 m
    sim = make_sim("A", keep=True, state=state)
    ref = REF.Totals(sim.engine.mfp_grid)
    sim.timestep(collect_paths=False)
    ref.add_step(sim.engine.drain_paths(sort=False), sim.engine.download())
    assert ref.bad is not None
    with pytest.raises(ArgonMCError) as e:
        sim.free_paths()
    assert e.value.code == AMC_ERR_CAPACITY and f"particle {ref.bad} " in str(e.value)
    sim.timestep(collect_paths=False)               # later steps add nothing
    with pytest.raises(ArgonMCError) as e:
        sim.free_paths()
    assert e.value.code == AMC_ERR_CAPACITY and f"particle {ref.bad} " in str(e.value)
    sim.free_paths_reset()
    tot, hist, counters = sim.engine.mfp_read()
    assert counters == (0, 0, 0) and not tot.any() and not hist.any()
    # the records of the faulted steps were skipped, not kept for later: a fresh state then samples as usual
    sim.engine.drain_paths()
    sim.set_state(*MS.initial_state("A"))
    ref = REF.Totals(sim.engine.mfp_grid)
    sim.timestep(collect_paths=False)
    ref.add_step(sim.engine.drain_paths(sort=False), sim.engine.download())
    check(sim.engine, ref)
    assert ref.n_records > 0
    sim.close()


def test_an_overflowed_record_buffer_marks_the_totals_lost_and_consuming_keeps_a_small_buffer_complete():
    assert_scenario_has_work("C")
    sim = make_sim("C", keep=True, max_paths=64)
    sim.timestep(collect_paths=False)               # 3,024 paths into 64 records
    with pytest.raises(ArgonMCError) as e:
        sim.free_paths()
    assert e.value.code == AMC_ERR_STATE and "lost" in str(e.value)
    sim.engine.drain_paths()
    sim.free_paths_reset()
    tot, hist, counters = sim.engine.mfp_read()
    assert counters == (0, 0, 0) and not tot.any() and not hist.any()
    sim.close()
    sim = make_sim("C", keep=False, max_paths=4096)
    sim.run(MS.STEPS["C"])
    check(sim.engine, reference("C", sim.engine.mfp_grid))
    sim.close()


def test_calls_before_a_config_and_without_records_return_state_errors():
    sim = make_sim("B", grid=None)
    for call in (sim.engine.mfp_reset, sim.engine.mfp_read, sim.free_paths):
        with pytest.raises(ArgonMCError) as e:
            call()
        assert e.value.code == AMC_ERR_STATE
    assert sim.engine.lib.amc_mfp_read(sim.engine._ctx, None, None, None, None, None) == AMC_ERR_STATE
    sim.close()
    sim = make_sim("B", grid=None, max_paths=-1)    # histograms only: no records to read
    with pytest.raises(ArgonMCError) as e:
        sim.enable_free_paths()
    assert e.value.code == AMC_ERR_STATE and "max_paths" in str(e.value)
    sim.close()


def test_a_consuming_config_behind_an_overflowed_record_buffer_starts_clean():
    """A run nobody drained has filled the record buffer (3,024 paths into 256 records); a consuming sampler configured then
    empties it and bins the next step's 186 paths, none lost.  With keep_records the same call needs a drain first."""
    assert_scenario_has_work("C")
    for keep in (False, True):
        sim = make_sim("C", grid=None, max_paths=256)
        sim.run(1)
        assert sim.engine.paths_pending() == 256
        sim.enable_free_paths(keep_records=keep)
        assert sim.engine.paths_pending() == (256 if keep else 0)
        sim.run(1)
        if keep:
            with pytest.raises(ArgonMCError) as e:
                sim.free_paths()
            assert e.value.code == AMC_ERR_STATE and "lost" in str(e.value)
        else:
            ref = reference("C", sim.engine.mfp_grid, 1, 2)
            check(sim.engine, ref)
            assert ref.n_records + ref.n_outside == 186
        sim.close()


def test_the_library_refuses_grids_the_python_layer_would_not_build():
    """amc_mfp_config's own checks, on hand-built structs: the column limit (6,144 accepted, one bin more refused), hist_bins,
    keep_records, hist_hi, reserved, struct_size and the fields' grid rules; a refused grid leaves the configured one on."""
    import ctypes as C
    from argon_monte_carlo_amd._abi import AMC_ERR_INVALID
    sim = make_sim("A", grid=None)
    p = sim.params
    good = FP.make_grid("cartesian", (8, 8, 6), (0.0, 0.0, 0.0), (p.cube_x, p.cube_y, p.cube_z), hist_bins=0)      # 384 x 2 x 8 = 6,144
    sim.engine.mfp_config(good)

    def refused(**change):
        g = FP.copy_grid(good)
        for k, v in change.items():
            setattr(g, k, v)
        with pytest.raises(ArgonMCError) as e:
            sim.engine.mfp_config(g)
        assert e.value.code == AMC_ERR_INVALID, change
        return str(e.value)

    assert "6,144" in refused(n3=7)                                 # 448 bins x 16 columns
    refused(hist_bins=1)                                            # 384 x 2 x 9
    refused(n1=43, n2=1, n3=1, hist_bins=64, hist_hi=1e-6)          # 43 x 2 x 72 = 6,192
    assert "hist_bins" in refused(hist_bins=65, n1=1, n2=1, n3=1) and "hist_bins" in refused(hist_bins=-1)
    assert "keep_records" in refused(keep_records=2)
    for bad in (0.0, -1e-6, float("inf"), float("nan")):
        assert "hist_hi" in refused(n1=1, n2=1, n3=1, hist_bins=8, hist_hi=bad)
    assert "reserved" in refused(reserved=1)
    assert "struct_size" in refused(struct_size=C.sizeof(type(good)) - 8)
    refused(kind=2)
    refused(n1=0)
    assert bytes(sim.engine.mfp_grid) == bytes(good)                # the grid configured before is still the one in force
    sim.timestep(collect_paths=False)
    assert sim.engine.mfp_read()[2][2] == 1
    g = FP.copy_grid(good)
    g.n1, g.n2, g.n3, g.hist_bins, g.hist_hi = 42, 1, 1, 64, 1e-6   # 42 x 2 x 72 = 6,048: accepted
    sim.engine.mfp_config(g)
    sim.close()


def test_write_free_paths_stores_the_derived_dict(tmp_path):
    assert_scenario_has_work("B")
    sim = make_sim("B", keep=False)
    sim.run(MS.STEPS["B"])
    f = sim.free_paths()
    path = str(tmp_path / "mfp.npz")
    sim.write_free_paths(path)
    z = np.load(path)
    assert set(z.files) == (set(f) - {"edges"}) | {"edges_1", "edges_2"}
    for k in z.files:
        want = f["edges"][int(k[-1]) - 1] if k.startswith("edges_") else f[k]
        assert np.array_equal(z[k], np.asarray(want), equal_nan=True), k
    assert np.array_equal(z["totals"], reference("B", sim.engine.mfp_grid).words()) and int(z["n_steps"]) == 7
    sim.close()


# ---- 5. entry points behind what a step leaves pending ---------------------------------------------------------------------------
def _produce(sim, how, k):
    if how == "timestep":
        for _ in range(k):
            sim.timestep(collect_paths=False)
    elif how == "run":
        sim.run(k)
    else:                               # one rank over the whole range: amc_mg_local, amc_mg_sweep(1, 0), amc_mg_finish(ctx, NULL)
        from argon_monte_carlo_amd.dist import LocalRanks
        job = LocalRanks([sim.engine])
        for _ in range(k):
            job.step(sim.dt)


@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("how", ["timestep", "run", "shard1"])
@pytest.mark.parametrize("consumer", ["config", "read", "load", "reset", "drain", "reset_outputs"])
def test_entry_points_behind_a_pending_step(name, how, consumer):
    """Three steps (single steps, one amc_run, or the sharded step's calls on one rank that owns everything, whose
    amc_mg_finish(ctx, NULL) returns without reading anything: in the cube all end with the sweep's results deferred and,
    without the sampler's own settling, its commit pending), then the entry point, then the remaining steps one by one.  The totals are
    the reference's over the steps the entry point leaves standing, the records of a drain or amc_reset_outputs between two
    steps are neither lost nor counted twice, and the trajectory is the undisturbed one."""
    assert_scenario_has_work(name)
    k, n = 3, MS.STEPS[name]
    sim = make_sim(name, keep=True, shard=how == "shard1")
    g = sim.engine.mfp_grid
    _produce(sim, how, k)
    first = 0
    if consumer == "config":
        sim.enable_free_paths(g, keep_records=True)
        first = k
    elif consumer == "read":
        check(sim.engine, reference(name, g, 0, k))
    elif consumer == "load":
        tot, hist, counters = sim.engine.mfp_read()
        sim.engine.mfp_reset()
        sim.engine.mfp_load(tot, hist, counters)
    elif consumer == "reset":
        sim.free_paths_reset()
        first = k
    elif consumer == "drain":
        rec = sim.engine.drain_paths(sort=False)
        assert len(rec) == sum(len(r) for r, _ in trace(name)["steps"][:k])
    else:
        sim.engine.reset_outputs()
    for _ in range(n - k):
        sim.timestep(collect_paths=False)
    ref = reference(name, g, first, n)
    check(sim.engine, ref)
    assert ref.n_records > 0
    want = sum(len(r) for r, _ in trace(name)["steps"][(0 if consumer in ("config", "read", "load", "reset") else k):])
    assert sim.engine.paths_pending() == want       # (keep mode: the records stay, from the last emptying on)
    st = sim.engine.download()
    for key in KEYS:
        assert np.array_equal(st[key], trace(name)["state"][key]), key
    sim.close()


# ---- 6. checkpoint ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep", [False, True])
def test_checkpoint_resume_gives_the_same_totals(keep, tmp_path):
    assert_scenario_has_work("B")
    sim = make_sim("B", keep=keep)
    g = sim.engine.mfp_grid
    sim.run(3)
    ck = str(tmp_path / "ck.npz")
    sim.save_checkpoint(ck)
    check(sim.engine, reference("B", g, 0, 3))      # (saving changed nothing)
    sim.close()
    p, c, kind = MS.scenario_params("B")
    res = Simulation(kind=kind, params=p, consts=c)
    res.load_checkpoint(ck)
    assert bytes(res.engine.mfp_grid) == bytes(g)
    res.run(4)
    ref = reference("B", g)
    check(res.engine, ref)
    assert ref.n_steps == 7 and ref.n_records > 0
    st = res.engine.download()
    for key in KEYS:
        assert np.array_equal(st[key], trace("B")["state"][key]), key
    res.close()


# ---- 7. the energised pore ---------------------------------------------------------------------------------------------------------
TEMP_STEPS = 6


def _temp_sim(mfp, surface=True):
    from argon_monte_carlo_amd.sim import TemperatureSimulation
    sim = TemperatureSimulation(n=20_000, device_rng_seed=17)
    sim.set_state(*MS.energised_state(20_000))
    if surface:
        sim.enable_surface()
    if mfp is not None:
        sim.enable_free_paths(keep_records=mfp)
    return sim


def test_energised_pore_run_equals_single_steps_and_reference():
    one = _temp_sim(True)
    ref = REF.Totals(one.engine.mfp_grid)
    wall = 0
    for _ in range(TEMP_STEPS):
        one.timestep(collect_paths=False)
        state = one.engine.download()
        rec = one.engine.drain_paths(sort=False)
        wall += int((REF.owners_and_kinds(rec)[1] == 0).sum())
        ref.add_step(rec, state)
    assert wall >= 1 and ref.n_records > wall       # the drain shows wall-ended paths (and p-p ones)
    tot = check(one.engine, ref)
    assert tot[:, 0, 0, 0].sum() > 0                # ... and they were binned as such
    surf = one.engine.surface_read()
    state = one.engine.download()
    one.close()
    for keep in (True, False):
        run = _temp_sim(keep)
        run.run(TEMP_STEPS)
        check(run.engine, ref)
        if keep:
            assert run.engine.paths_pending() == ref.n_records + ref.n_outside
        else:
            assert run.engine.paths_pending() == 0
        s = run.engine.surface_read()
        assert all(np.array_equal(u, v) for u, v in zip(s[:2], surf[:2])) and s[2] == surf[2] == TEMP_STEPS
        st = run.engine.download()
        for key in KEYS:
            assert np.array_equal(st[key], state[key]), key
        run.close()
    bare = _temp_sim(None)                          # the surfaces without the free paths beside them
    bare.run(TEMP_STEPS)
    s = bare.engine.surface_read()
    assert all(np.array_equal(u, v) for u, v in zip(s[:2], surf[:2])) and s[2] == TEMP_STEPS and s[0].any()
    bare.close()


# ---- 8. shards on one GPU ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lo,hi", ODD_SHARDS)
def test_a_context_with_an_odd_index_range_bins_the_records_it_emitted(lo, hi):
    """One ShardEngine over [lo, hi) of scenario B stepped by amc_timestep: only its own particles move, and every record it
    emits has its owner in the range."""
    from argon_monte_carlo_amd.engine import ShardEngine
    p, c, _ = MS.scenario_params("B")
    p.reserved1 = 1                                 # (a long step: tolerate the events where the reference raises FloatingPointError)
    eng = ShardEngine(p, lo, hi)
    s = MS.initial_state("B")
    eng.upload(*s[:10], flag=s[10])
    eng.mfp_config(FP.default_grid(p, keep_records=True))
    ref = REF.Totals(eng.mfp_grid)
    owners = []
    for _ in range(12):
        eng.timestep(40 * c["dt"])                  # (2,000 movers: a longer step brings the walls within reach)
        state = eng.download()
        rec = eng.drain_paths(sort=False)
        owners.extend(REF.owners_and_kinds(rec)[0].tolist())
        ref.add_step(rec, state)
    assert ref.n_records > 0 and all(lo <= o < hi for o in owners)
    check(eng, ref)
    eng.close()


class _Captured(Exception):
    pass


class _CaptureComm:
    """records what a rank would contribute to the all-reduce"""
    shortcut = False

    def allreduce_sum_ints(self, values):
        self.values = [int(v) for v in values]
        raise _Captured


class _SumComm:
    shortcut = False

    def __init__(self, rows):
        self.sums = [sum(col) for col in zip(*rows)]

    def allreduce_sum_ints(self, values):
        assert len(values) == len(self.sums)
        return list(self.sums)


def _ranks_free_paths(p, engs, dt):
    """ShardedSimulation.free_paths() of every rank of an in-process job: the all-reduce is the sum of what each rank hands it"""
    from argon_monte_carlo_amd.dist import ShardedSimulation
    world = len(engs)
    rows = []
    for r, e in enumerate(engs):
        comm = _CaptureComm()
        with pytest.raises(_Captured):
            ShardedSimulation(p, r, world, engine=e, comm=comm).free_paths(dt)
        rows.append(comm.values)
    out = []
    for r, e in enumerate(engs):
        try:
            out.append(ShardedSimulation(p, r, world, engine=e, comm=_SumComm(rows)).free_paths(dt))
        except ArgonMCError as err:
            out.append(err)
    return out


@pytest.mark.parametrize("world", [2, 3])
def test_ranks_on_one_gpu_sum_to_the_single_context(world):
    """Scenario B over the driver's own shards (the step protocol pins a rank's range to them; three ranks cut at the odd
    indices 6,667 and 13,334): the ranks' totals, histograms and counters summed by totals.sum_over_ranks equal the single
    context's bit for bit, and a path out of range on one rank raises on every rank."""
    from argon_monte_carlo_amd.dist import LocalRanks, shard_range
    from argon_monte_carlo_amd.engine import ShardEngine
    assert_scenario_has_work("B")
    p, c, _ = MS.scenario_params("B")
    stream = torch.cuda.current_stream().cuda_stream
    engs = [ShardEngine(p, *shard_range(int(p.n), r, world)) for r in range(world)]
    s = MS.initial_state("B")
    for e in engs:
        e.set_stream(stream)
        e.upload(*s[:10], flag=s[10])
        e.mfp_config(FP.default_grid(p))
    job = LocalRanks(engs)
    for _ in range(MS.STEPS["B"]):
        job.step(c["dt"])
    ref = reference("B", engs[0].mfp_grid)
    per_rank = [e.mfp_read() for e in engs]
    assert sum(r[2][0] for r in per_rank) == ref.n_records and all(r[2][2] == 7 for r in per_rank)
    assert sum(1 for r in per_rank if r[2][0] > 0) >= 2         # more than one rank has binned something
    for f in _ranks_free_paths(p, engs, c["dt"]):
        assert np.array_equal(f["totals"], ref.words()) and np.array_equal(f["hist_totals"], ref.hist)
        assert (f["n_records"], f["n_outside"], f["n_steps"]) == ref.counters()
    # a path out of range on the last rank: every rank raises, naming the particle
    bad = list(MS.initial_state("B"))
    lo, hi = shard_range(int(p.n), world - 1, world)
    bad[6] = np.where(np.arange(int(p.n)) >= lo, 1e-4, 0.0)
    for e in engs:
        e.upload(*bad[:10], flag=bad[10])
        e.mfp_reset()
    for _ in range(MS.STEPS["B"]):
        job.step(c["dt"])
    with pytest.raises(ArgonMCError) as own:
        engs[-1].mfp_read()
    assert own.value.code == AMC_ERR_CAPACITY
    engs[0].mfp_read()                                           # (the first rank's own read is fine)
    outs = _ranks_free_paths(p, engs, c["dt"])
    assert all(isinstance(o, ArgonMCError) and o.code == AMC_ERR_CAPACITY for o in outs)
    named = {str(o).split("particle ")[1].split(" ")[0] for o in outs}
    assert len(named) == 1 and lo <= int(named.pop()) < hi
    for e in engs:
        e.close()
