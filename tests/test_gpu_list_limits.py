"""GPU (-m gpu): the kept per-cell lists (amc_list_keep, amc_grid_dev.h; amc_list_build_mode, amc_stream.hip) at each of their
limits, on the crafted movers of tests/list_states.py.  Bar: bit for bit equal to the oracle (`mul`) after every call — state,
counters including n_candidates, completed-path records — and, through Engine.lists_stats(), proof that the limit was reached:
the cycle's age, the sum and the maximum of the waves' pool counters and the number of full builds equal the host mirror's
after every call; the marching waves stand at wave_cap exactly on the last step in between and nothing overflows.

The oracle's runs are made once per state (the module-scoped ``runs``), together with the catalogue's proofs
(tests/test_list_states_host.py asserts them on the CPU for every combination); block sizes replay them."""
import numpy as np
import pytest

from tests import list_states as LS
from tests.test_gpu_edges import Engine, O, assert_records_equal, assert_state_equal  # noqa: F401  (Engine, O: fixtures)

pytestmark = pytest.mark.gpu

# calls per cycle length: timestep() and run(k) mixed, boundaries inside the cycles and right behind the last step in between
# of either cycle (after K and after 2 K steps); every run is shorter than the on-demand run's threshold of 8 steps
CHUNKS = {2: (1, 1, 2, 1), 3: (1, 2, 1, 2, 1), 4: (1, 3, 2, 2, 1), 8: (1, 2, 5, 3, 5, 1)}


@pytest.fixture(scope="module")
def runs(O):
    memo = {}

    def get(kind, perm, cell, K):
        key = (kind, perm, cell, K)
        if key not in memo:
            s = LS.catalogue(kind, perm, cell, K)
            run = LS.oracle_run(O, s, LS.steps(K))
            memo[key] = (run,) + LS.catalogue_proofs(s, run)
        return (LS.catalogue(kind, perm, cell, K),) + memo[key]
    return get


def _engine(Engine, s):
    eng = Engine(s.p)
    a = s.arrays()
    eng.upload(*a[:10], flag=a[10])
    return eng


def _check_call(eng, st, results, ctx, candidates=None):
    """one call of the engine against the oracle's steps it covers"""
    for key in LS.COUNTERS:
        assert st[key] == sum(r["stats"][key] for r in results), (ctx, key, st)
    assert not st["flags"] & 9, (ctx, st)                       # neither the pools' overflow nor a particle outside its window
    if candidates is not None:
        assert st["n_candidates"] == candidates, (ctx, st, candidates)
    assert_state_equal(eng.download(), results[-1]["state"], ctx)
    assert_records_equal(eng.drain_paths(), np.concatenate([r["rec"] for r in results]), ctx)


def _check_lists(eng, want, K, n, bs, ctx, owner=1):
    ls = eng.lists_stats()
    print(ctx, ls)
    assert (ls["keep_K"], ls["wave_cap"], ls["owner"]) == (K, 64 * (K - 1), owner), (ctx, ls)
    assert ls["waves"] == -(-n // bs) * (bs // 64), (ctx, ls)
    assert (ls["lists_age"], ls["count_sum"], ls["count_max"], ls["full_builds"]) == want, (ctx, ls, want)
    return ls


# ---------------------------------------------------------------------------------------------------------------- cycles
@pytest.mark.parametrize("bs", [256, 64])
@pytest.mark.parametrize("K", LS.KS)
@pytest.mark.parametrize("cell", LS.CELLS)
@pytest.mark.parametrize("kind", LS.KINDS)
def test_two_cycles_and_a_step_equal_the_oracle_and_the_mirror(Engine, runs, monkeypatch, kind, cell, K, bs):
    monkeypatch.setenv("AMC_LIST_KEEP", str(K))
    if bs != 256:
        monkeypatch.setenv("AMC_STREAM_BS", str(bs))
    for perm in LS.PERMS:
        s, run, counts, ncand = runs(kind, perm, cell, K)
        want = LS.expected_stats(counts, K)
        eng = _engine(Engine, s)
        t = 0
        for k in CHUNKS[K]:
            ctx = (kind, perm, cell, K, bs, "steps", t, t + k)
            st = eng.run(s.dt, k) if k > 1 else eng.timestep(s.dt)
            _check_call(eng, st, run[t:t + k], ctx, sum(ncand[t:t + k]))
            t += k
            ls = _check_lists(eng, want[t - 1], K, s.n, bs, ctx)
            if t in (K, 2 * K):                     # the last step in between: the marching waves have used their pools up
                assert ls["count_max"] == ls["wave_cap"], (ctx, ls)
        assert t == LS.steps(K)
        eng.close()


@pytest.mark.parametrize("cell", LS.CELLS)
@pytest.mark.parametrize("kind", LS.KINDS)
def test_face_rounding_equals_the_oracle(Engine, O, monkeypatch, kind, cell):
    """a particle whose single-precision record is on a grid face while its double position is below it: the physics only"""
    monkeypatch.setenv("AMC_LIST_KEEP", "4")
    s = LS.face_rounding(kind, cell)
    run = LS.oracle_run(O, s, LS.steps(4))
    LS.catalogue_proofs(s, run)
    eng = _engine(Engine, s)
    t = 0
    for k in CHUNKS[4]:
        st = eng.run(s.dt, k) if k > 1 else eng.timestep(s.dt)
        _check_call(eng, st, run[t:t + k], (kind, cell, t))
        t += k
    eng.close()


# ---------------------------------------------------------------------------------------------------------------- cycles that must end
def _stage_step(eng, s):
    pore = s.p.geometry != 1
    eng.stage_drift(s.dt)
    eng.stage_walls()
    if pore:
        eng.stage_bounds()
    eng.stage_sweep()
    if pore:
        eng.stage_bounds()


@pytest.mark.parametrize("how", ["stage_calls", "partial_upload", "load_checkpoint", "init_synthetic"])
@pytest.mark.parametrize("kind", LS.KINDS)
def test_an_interrupted_cycle_starts_with_a_full_build(Engine, O, monkeypatch, tmp_path, kind, how):
    """Two steps into a cycle of four, pool nodes live: an entry point that replaces state or builds lists of its own ends
    the cycle.  lists_stats() shows no cycle afterwards and a fresh full build at the next step; the following 2 K steps
    equal the oracle, with the counters of a mirror that starts at that full build."""
    K = 4
    monkeypatch.setenv("AMC_LIST_KEEP", str(K))
    s = LS.catalogue(kind, "identity", "min", K)
    tape = LS.Tape(O, s)
    eng = _engine(Engine, s)
    for t in range(2):
        _check_call(eng, eng.timestep(s.dt), [tape.step()], (kind, how, "before", t))
    ls = eng.lists_stats()
    assert ls["lists_age"] == 1 and ls["count_sum"] > 0 and ls["full_builds"] == 1, ls
    crafted = True
    if how == "stage_calls":
        _stage_step(eng, s)
        r = tape.step()
        assert_state_equal(eng.download(), r["state"], (kind, how))
        assert_records_equal(eng.drain_paths(), r["rec"], (kind, how))
    elif how == "partial_upload":
        eng.upload(x=tape.state()["x"])
    elif how == "load_checkpoint":
        from argon_monte_carlo_amd.sim import Simulation
        sim = Simulation(kind, params=s.p, consts=dict(s.extra["consts"]), engine=eng)
        path = str(tmp_path / "mid_cycle.npz")
        sim.save_checkpoint(path)
        held = tape.state()
        eng.timestep(s.dt)                          # (one step further into the cycle, then back to the checkpoint)
        assert eng.lists_stats()["lists_age"] == 2
        sim.load_checkpoint(path)
        tape.set_state(held)
        eng.drain_paths()
    else:
        from argon_monte_carlo_amd import ic as IC
        eng.init_synthetic(IC.device_ic_config(s.p, s.extra["consts"], 77, kind))
        tape.set_state(eng.download())
        eng.drain_paths()
        crafted = False                             # (a random gas: its candidate count is the detector's own business)
    ls = eng.lists_stats()
    assert ls["lists_age"] == -1 and ls["full_builds"] == 1, (kind, how, ls)
    pre, results = [], []
    for j in range(2 * K):
        st = eng.timestep(s.dt)
        r = tape.step()
        pre.append(r["pre"])
        pairs, band = LS.close_pairs(s, r["pre"])
        if crafted:                                 # (these steps reach past the 2 K + 1 the catalogue's proofs cover)
            assert band.size == 0, (kind, how, j, band)
        _check_call(eng, st, [r], (kind, how, "after", j), len(pairs) if crafted else None)
        counts, outside = LS.movers_per_wave(s.p, s.extra["h_asked"], pre, K)
        assert not outside.any()
        age, total, top, builds = LS.expected_stats(counts, K)[-1]
        _check_lists(eng, (age, total, top, 1 + builds), K, s.n, 256, (kind, how, "after", j))
    eng.close()


# ---------------------------------------------------------------------------------------------------------------- energised pore
@pytest.mark.parametrize("K", [2, 4])
@pytest.mark.parametrize("cell", LS.CELLS)
def test_energised_pore_files_the_same_lists(runs, monkeypatch, cell, K):
    """The marching waves, the pool-pool pairs and the layer window in the energised pore, far from every energised surface,
    through TemperatureSimulation with the draws on the device: single steps file the lists in amc_temp_end's bounds pass,
    run(k) in the fused pass.  Equal to the energised oracle (no case fires: nothing random is left), same lists_stats()."""
    from argon_monte_carlo_amd.sim import TemperatureSimulation
    monkeypatch.setenv("AMC_GAP_WORKERS", "0")
    monkeypatch.setenv("AMC_LIST_KEEP", str(K))
    for perm in LS.PERMS:
        s, run, counts, ncand = runs("temp", perm, cell, K)
        assert {"march_full", "pair_pool_pool", "layer_window"} <= set(s.cases)
        want = LS.expected_stats(counts, K)
        sim = TemperatureSimulation(params=s.p, consts=s.extra["consts"], device_rng_seed=11)
        try:
            a = s.arrays()
            sim.set_state(*a[:10], a[10])
            t = 0
            for k in CHUNKS[K]:
                ctx = ("temp", perm, cell, K, "steps", t, t + k)
                st = sim.run(k) if k > 1 else sim.timestep(collect_paths=False)
                _check_call(sim.engine, st, run[t:t + k], ctx, sum(ncand[t:t + k]))
                t += k
                ls = _check_lists(sim.engine, want[t - 1], K, s.n, 256, ctx)
                if t in (K, 2 * K):
                    assert ls["count_max"] == ls["wave_cap"], (ctx, ls)
        finally:
            sim.close()


# ---------------------------------------------------------------------------------------------------------------- sharded
# where the first shard boundary falls relative to the 192 marching particles [shift, shift + 192): (world, shift, pad)
SHARDED = {"inside_a_marching_wave": (2, 640, 35), "at_a_multiple_of_64": (3, 320, 27), "one_before_a_wave_ends": (3, 320, 24)}
SHARDED_K = 4


def _sharded_worker(rank, world, port, shift, pad, q):
    import os

    import torch.distributed as dist
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        try:
            from argon_monte_carlo_amd.dist import ShardedSimulation
            s = LS.catalogue("pore", "identity", "min", SHARDED_K, shift, pad)
            sim = ShardedSimulation(s.p, rank, world, backend="gloo")
            a = s.arrays()
            sim.upload(*a[:10], flag=a[10])
            per_step = []
            for _ in range(LS.steps(SHARDED_K)):
                st = sim.timestep(s.dt)
                per_step.append((st, sim.engine.lists_stats(), sim.download()))
            sim.upload(*a[:10], flag=a[10])             # (ends the cycle: the figures stay the exchange kernels')
            ended = sim.engine.lists_stats()
            sim.engine.close()
            everybody = [None] * world
            dist.all_gather_object(everybody, (per_step, ended))
            if rank == 0:
                q.put(("ok", everybody))
        finally:
            dist.destroy_process_group()
    except BaseException as e:
        import traceback
        q.put(("error", f"rank {rank}: {e!r}\n{traceback.format_exc()}"))
        raise


@pytest.mark.parametrize("where", list(SHARDED))
def test_sharded_ranks_file_the_same_lists_in_the_exchange_kernels(Engine, O, monkeypatch, where):
    """Ranks on one GPU, the pore: the lists are filed by k_kin_pack (the own shard) and k_kin_unpack (the others), the pools
    are theirs and lists_stats() reports owner 2.  Every rank's state equals the oracle's (and the single engine's) after
    every step, its counters the mirror's for its own waves; the marching waves reach wave_cap and do not pass it."""
    from argon_monte_carlo_amd.dist import shard_range
    from tests.test_gpu_dist import _run_ranks
    world, shift, pad = SHARDED[where]
    K = SHARDED_K
    monkeypatch.setenv("AMC_LIST_KEEP", str(K))
    s = LS.catalogue("pore", "identity", "min", K, shift, pad)
    lo1 = shard_range(s.n, 1, world)[0]
    assert shift < lo1 < shift + 64 * LS.FULL_WAVES, (lo1, shift)
    at = (lo1 - shift) % 64
    assert {"inside_a_marching_wave": 0 < at < 63, "at_a_multiple_of_64": at == 0 and lo1 % 64 == 0,
            "one_before_a_wave_ends": at == 63}[where], (where, lo1, shift)
    run = LS.oracle_run(O, s, LS.steps(K))
    LS.catalogue_proofs(s, run)
    # the single engine on the same state
    eng = _engine(Engine, s)
    for t, r in enumerate(run):
        _check_call(eng, eng.timestep(s.dt), [r], (where, "single engine", t))
    eng.close()
    everybody = _run_ranks(world, (shift, pad), target=_sharded_worker)
    assert len(everybody) == world
    pre = [r["pre"] for r in run]
    for rank, (per_step, ended) in enumerate(everybody):
        wave, nwaves = LS.exchange_waves(s.n, world, rank)
        counts, outside = LS.movers_per_wave(s.p, s.extra["h_asked"], pre, K, wave=wave, nwaves=nwaves)
        want = LS.expected_stats(counts, K)
        assert not outside.any() and counts[K - 1].max() == 64 * (K - 1)
        for t, (st, ls, state) in enumerate(per_step):
            ctx = (where, "rank", rank, "step", t)
            print(ctx, ls)
            for key in LS.COUNTERS:
                assert st[key] == run[t]["stats"][key], (ctx, key, st)
            assert not st["flags"] & 9, (ctx, st)
            assert_state_equal(state, run[t]["state"], ctx)
            assert (ls["keep_K"], ls["wave_cap"], ls["owner"], ls["waves"]) == (K, 64 * (K - 1), 2, nwaves), (ctx, ls)
            assert (ls["lists_age"], ls["count_sum"], ls["count_max"], ls["full_builds"]) == want[t], (ctx, ls, want[t])
            if t in (K - 1, 2 * K - 1):
                assert ls["count_max"] == ls["wave_cap"], (ctx, ls)
        last = per_step[-1][1]
        assert (ended["lists_age"], ended["owner"], ended["full_builds"]) == (-1, 0, last["full_builds"]), (rank, ended)
        assert (ended["waves"], ended["count_sum"], ended["count_max"]) == (nwaves, last["count_sum"], last["count_max"]), (rank, ended)
