"""The ordered workgroup on demand: inside amc_run the steps are enqueued without k_resolve<GEOM,0>; a sweep
that needs it stalls the later steps, the host launches it for that sweep and enqueues the later steps again.  Whatever
the share of such sweeps, the run computes what the oracle computes bit for bit — state, counters, completed paths,
histograms — and what AMC_ORDERED_ALWAYS=1 (the workgroup in every sweep) computes."""
import numpy as np
import pytest

from argon_monte_carlo_amd import ic as IC
from argon_monte_carlo_amd import params as PR
from tests.test_gpu_parity import assert_state_equal, paths_of

pytestmark = pytest.mark.gpu

# what a step computes.  (n_rounds and n_clusters count how the sweep was divided between the wide kernel and the ordered
# workgroup: that follows the launch plan, which is chosen from a candidate count the host reads without synchronisation
# — they differ between two runs of one mode as well.)
COUNTERS = ("n_pp", "n_wall", "n_oob_walls", "n_oob_pp", "n_paths", "n_fp_errors", "n_candidates")


@pytest.fixture(scope="module")
def Engine():
    from argon_monte_carlo_amd.engine import Engine as E
    return E


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def bench_like(kind, n):
    if kind == "cube":
        p, c = PR.cube_params_for_n(n)
        init = IC.cube_ic(p, c, seed=127)
    else:
        p, c = PR.pore_params(n=n)
        init = IC.pore_ic(p, c, seed=17)
    p.reserved1 = 1
    return p, c["dt"], init


def stress(kind, n, sigma_mult):
    """The high-collision inputs of test_gpu_parity.test_high_collision_rate_stresses_the_wide_cluster_kernel."""
    sigma = 3.6e-19 * sigma_mult
    if kind == "cube":
        p, c = PR.cube_params_for_n(n, sigma=sigma)
        init = IC.cube_ic(p, c, seed=41)
    else:
        p, c = PR.pore_params(n=n, sigma=sigma)
        init = IC.pore_ic(p, c, seed=41)
    p.detect_mode = 1
    p.reserved1 = 1
    return p, c["dt"], init


def dense_blob():
    """The dense blob of test_gpu_parity.test_dense_cluster_chains_match_oracle (volume fraction ~20 %), grid detector."""
    n = 400
    rng = np.random.default_rng(99)
    p, c = PR.cube_params(n=n)
    p.detect_mode = 1
    cr = p.collision_range
    side = (n * (4.0 / 3.0) * np.pi * (cr / 2) ** 3 / 0.2) ** (1.0 / 3.0)
    pos = rng.random((3, n)) * side + 40e-9
    vel = rng.normal(size=(3, n)) * 250.0
    return p, 2.0e-14, (pos[0], pos[1], pos[2], vel[0], vel[1], vel[2])


def run_chunks(Engine, p, dt, init, chunks):
    """Engine through amc_run in the given chunks: (stats per chunk, state, histograms, sorted paths, overlap_stats)."""
    eng = Engine(p)
    eng.upload(*init)
    stats = [eng.run(dt, k) for k in chunks]
    out = (stats, eng.download(), eng.histograms(), paths_of(eng.drain_paths()), eng.overlap_stats())
    eng.close()
    return out


def oracle_chunks(O, p, dt, init, chunks):
    orc = O.Oracle(p, mode="mul", path_capacity=1 << 22)
    orc.upload(*init)
    sums = []
    for k in chunks:
        so = {}
        for _ in range(k):
            rc, s1 = orc.timestep(dt)
            assert rc == 0
            for key in ("n_pp", "n_wall", "n_oob_walls", "n_oob_pp", "n_paths", "n_fp_errors"):
                so[key] = so.get(key, 0) + s1[key]
        sums.append(so)
    ref = orc.paths()
    exp = np.stack([ref["total"], ref["px"], ref["py"], ref["pz"]], axis=1) if len(ref["total"]) else np.zeros((0, 4))
    return sums, orc.state(), exp


def assert_histograms_equal_oracle(p, hist, ref_paths, ctx):
    """The device histograms against np.histogram of the oracle's completed paths (total, x, y, z), as tests/soak.py does."""
    counts, npaths = hist
    assert npaths == len(ref_paths), (ctx, npaths, len(ref_paths))
    for row in range(4):
        ref, _ = np.histogram(ref_paths[:, row], bins=p.hist_bins, range=(p.hist_lo, p.hist_hi))
        assert np.array_equal(counts[row], ref.astype(np.uint64)), (ctx, "histogram row", row)


def check_both_modes(Engine, O, monkeypatch, p, dt, init, chunks, ctx):
    """On demand and always: equal to the oracle and to each other.  Returns the two overlap_stats."""
    sums, ref_state, ref_paths = oracle_chunks(O, p, dt, init, chunks)
    res = {}
    monkeypatch.setenv("AMC_OD_MAX_N", "100000000")     # (on demand at every size, not only where it is the default)
    for always in ("0", "1"):
        monkeypatch.setenv("AMC_ORDERED_ALWAYS", always)
        stats, state, hist, paths, ov = run_chunks(Engine, p, dt, init, chunks)
        for st, so in zip(stats, sums):
            for k in so:
                assert st[k] == so[k], (ctx, always, k, st, so)
        assert_state_equal(state, ref_state, (ctx, always))
        assert paths.shape == ref_paths.shape, (ctx, always)
        assert np.array_equal(paths[np.lexsort(paths.T[::-1])], ref_paths[np.lexsort(ref_paths.T[::-1])]), (ctx, always)
        assert_histograms_equal_oracle(p, hist, ref_paths, (ctx, always))
        res[always] = (stats, state, hist, ov)
    for a, b in zip(res["0"][0], res["1"][0]):
        for k in COUNTERS:
            assert a[k] == b[k], (ctx, k, a, b)
    assert_state_equal(res["0"][1], res["1"][1], (ctx, "on demand vs always"))
    assert np.array_equal(res["0"][2][0], res["1"][2][0]) and res["0"][2][1] == res["1"][2][1], ctx
    return res["0"][3], res["1"][3]


@pytest.mark.parametrize("kind,n,steps", [("cube", 100_000, 120), ("pore", 300_000, 60)])
def test_run_equals_oracle_and_the_always_run(Engine, O, monkeypatch, kind, n, steps):
    """The bench workload's kind of run: nearly every sweep is resolved by the wide kernel alone.  The ordered workgroup
    is launched for fewer sweeps than there are steps; with the switch, for every one."""
    p, dt, init = bench_like(kind, n)
    od, al = check_both_modes(Engine, O, monkeypatch, p, dt, init, [steps], kind)
    assert al["ordered_launches"] == steps and al["on_demand_steps"] == 0, al
    assert 1 <= od["ordered_launches"] < steps, od
    assert od["ordered_launches"] <= od["stalls"] + 1, od      # (one per stall, and the run's last sweep)
    assert od["on_demand_steps"] >= steps, od


@pytest.mark.parametrize("n,on_demand", [(100_000, True), (100_001, False)])
def test_the_default_size_bound(Engine, monkeypatch, n, on_demand):
    """Without AMC_OD_MAX_N the plan applies up to N = 100,000: one particle more and amc_run launches the
    ordered workgroup in every sweep."""
    monkeypatch.delenv("AMC_OD_MAX_N", raising=False)
    monkeypatch.delenv("AMC_ORDERED_ALWAYS", raising=False)
    p, dt, init = bench_like("cube", n)
    eng = Engine(p)
    eng.upload(*init)
    eng.run(dt, 20)
    ov = eng.overlap_stats()
    eng.close()
    if on_demand:
        assert ov["on_demand_steps"] >= 20 and ov["ordered_launches"] < 20, ov
    else:
        assert ov["on_demand_steps"] == 0 and ov["ordered_launches"] == 20, ov


@pytest.mark.parametrize("wide_waves", [0, 4])
def test_dense_blob_every_step_stalls_and_resumes(Engine, O, monkeypatch, wide_waves):
    if wide_waves:
        monkeypatch.setenv("AMC_CW_BLOCKS", str(wide_waves))
    p, dt, init = dense_blob()
    od, al = check_both_modes(Engine, O, monkeypatch, p, dt, init, [12], ("dense", wide_waves))
    assert od["ordered_launches"] >= 6, od          # (most sweeps need the ordered pass)
    assert od["on_demand_steps"] > 12, od           # ... and the steps behind them were enqueued again


@pytest.mark.parametrize("kind,n,sigma_mult,wide_waves", [("cube", 30_000, 16.0, 0), ("pore", 60_000, 30.0, 0),
                                                         ("cube", 30_000, 16.0, 4), ("pore", 60_000, 30.0, 4)])
def test_high_collision_rate_stalls_and_resumes(Engine, O, monkeypatch, kind, n, sigma_mult, wide_waves):
    if wide_waves:
        monkeypatch.setenv("AMC_CW_BLOCKS", str(wide_waves))
    p, dt, init = stress(kind, n, sigma_mult)
    od, _ = check_both_modes(Engine, O, monkeypatch, p, dt, init, [16], ("stress", kind, wide_waves))
    assert od["ordered_launches"] >= 2, od


def test_a_run_whose_last_step_stalls(Engine, O, monkeypatch):
    """Runs of every length from 8 to 13 over the dense blob, whose sweeps nearly all stall: the last step's among them —
    found by the run's final synchronisation."""
    p, dt, init = dense_blob()
    at_last = 0
    for steps in range(8, 14):
        od, _ = check_both_modes(Engine, O, monkeypatch, p, dt, init, [steps], ("last", steps))
        assert od["ordered_launches"] == od["stalls"] + (0 if od["stalls_at_last_step"] else 1), od
        at_last += od["stalls_at_last_step"]
    assert at_last >= 1, at_last        # the case did occur


@pytest.mark.parametrize("kind,n,sigma_mult", [("cube", 30_000, 16.0), ("pore", 60_000, 30.0)])
def test_split_runs_with_a_timestep_and_an_upload_between(Engine, O, monkeypatch, kind, n, sigma_mult):
    """amc_run, amc_timestep, amc_run, download + upload of the same state, amc_run (short: the always plan), amc_run."""
    p, dt, init = stress(kind, n, sigma_mult)
    sums, ref_state, ref_paths = oracle_chunks(O, p, dt, init, [9, 1, 12, 3, 10])
    res = {}
    monkeypatch.setenv("AMC_OD_MAX_N", "100000000")
    for always in ("0", "1"):
        monkeypatch.setenv("AMC_ORDERED_ALWAYS", always)
        eng = Engine(p)
        eng.upload(*init)
        stats = [eng.run(dt, 9), eng.timestep(dt), eng.run(dt, 12)]
        st = eng.download()
        eng.upload(*[st[k] for k in ("x", "y", "z", "vx", "vy", "vz", "d", "dx", "dy", "dz")], st["flag"])
        stats += [eng.run(dt, 3), eng.run(dt, 10)]
        for got, so in zip(stats, sums):
            for k in so:
                assert got[k] == so[k], (kind, always, k, got, so)
        state, hist, paths = eng.download(), eng.histograms(), paths_of(eng.drain_paths())
        eng.close()
        assert_state_equal(state, ref_state, (kind, always))
        assert paths.shape == ref_paths.shape, (kind, always)
        assert np.array_equal(paths[np.lexsort(paths.T[::-1])], ref_paths[np.lexsort(ref_paths.T[::-1])]), (kind, always)
        assert_histograms_equal_oracle(p, hist, ref_paths, (kind, always))
        res[always] = (stats, hist)
    for a, b in zip(res["0"][0], res["1"][0]):
        for k in COUNTERS:
            assert a[k] == b[k], (kind, k, a, b)
    assert np.array_equal(res["0"][1][0], res["1"][1][0]) and res["0"][1][1] == res["1"][1][1]
