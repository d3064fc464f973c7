"""The host-free run of the energised pore in device-RNG mode (``amc_temp_run_device``) against the step-by-step
path it replaces (``EnergisedEngine.temp_timestep_device``, which test_device_rng_energised_walls_match_oracle_on_the_same_draws
pins to the oracle).  Every comparison is bitwise: the run does the same arithmetic in the same order.

The runs that need another set of environment switches (read when a context is created) happen in fresh child processes:
this file is its own child program, ``python -m tests.test_gpu_temp_run <job> <out.npz>``.

Order independence of the device sums (the kernel has no entry point of its own): the same run is repeated with the
streaming pass at another block size (AMC_STREAM_BS=64) and with the single step's kernels (AMC_TEMP_RUN_UNFUSED=1) — the hit
records are appended by other kernels, in other atomic orders — and the series has to come out the same."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from argon_monte_carlo_amd import ic as IC  # noqa: E402
from argon_monte_carlo_amd import params as PR  # noqa: E402
from argon_monte_carlo_amd.energised import CASES  # noqa: E402

pytestmark = pytest.mark.gpu

BIG_N, BIG_STEPS, BIG_SEED = 1_000_000, 20, 0x1234ABCD5678
STATE_KEYS = ("x", "y", "z", "vx", "vy", "vz", "d", "dx", "dy", "dz", "flag")
STAT_KEYS = ("n_pp", "n_wall", "n_oob_walls", "n_oob_pp", "n_paths", "n_candidates", "n_fp_errors")


def big_engine(n=BIG_N):
    from argon_monte_carlo_amd.energised import SurfaceEnergies, device_rng_config
    from argon_monte_carlo_amd.engine import EnergisedEngine
    p, c = PR.pore_params(n=n, energised=True)
    p.reserved0 |= 1
    init = IC.pore_ic(p, c, seed=29)
    cfg = device_rng_config(c, BIG_SEED)
    energies = SurfaceEnergies(c)
    p.E_cold, p.E_hot = energies.cold, energies.hot
    eng = EnergisedEngine(p)
    eng.upload(*init)
    return eng, cfg, c["dt"]


def snapshot(eng, stats, series, had):
    """Everything the issue lists, as a flat dict of arrays."""
    out = {f"state_{k}": v for k, v in eng.download().items()}
    out["prior"] = np.stack(eng.download_prior())
    out["stats"] = np.array([stats[k] for k in STAT_KEYS], dtype=np.int64)
    counts, tot = eng.histograms()
    out["hist"], out["hist_total"] = counts, np.array([tot], dtype=np.uint64)
    rec = eng.drain_paths(sort=True)
    out["paths"] = np.frombuffer(rec.tobytes(), dtype=np.uint8)
    out["series"], out["had"] = np.asarray(series, dtype=np.float64).reshape(-1, 3), np.asarray(had, dtype=bool).reshape(-1, 3)
    for case in CASES:
        for name, arrs in (("res", eng.device_results(case)), ("draw", eng.device_draws(case))):
            for k, a in enumerate(arrs):
                out[f"{name}_{case}_{k}"] = np.asarray(a)
    sums, hd = (C.c_double * 3)(), (C.c_int32 * 3)()
    eng._ck(eng.lib.amc_temp_device_sums(eng._ctx, sums, hd))
    out["last_sums"], out["last_had"] = np.array(list(sums)), np.array([bool(v) for v in hd])
    return out


def assert_same(a, b, what):
    assert sorted(a) == sorted(b), what
    for k in sorted(a):
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, (what, k, a[k].shape, b[k].shape)
        if a[k].dtype.kind == "f":
            assert np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)), (what, k)     # (bits: NaN and -0.0 included)
        else:
            assert np.array_equal(a[k], b[k]), (what, k)


def job_big_run(n=BIG_N):
    eng, cfg, dt = big_engine(n)
    st, series, had = eng.temp_run_device(dt, BIG_STEPS, cfg)
    snap = snapshot(eng, st, series, had)
    eng.close()
    return snap


def job_capacity():
    """With room for 8 records per case a step at N = 2e5 (about 17 hits per case) overflows: the run says which case."""
    from argon_monte_carlo_amd._lib import ArgonMCError
    eng, cfg, dt = big_engine(200_000)
    code, msg = 0, ""
    try:
        eng.temp_run_device(dt, 3, cfg)
    except ArgonMCError as e:
        code, msg = e.code, str(e)
    eng.close()                                     # (the context is destroyed cleanly after the failure)
    return {"code": np.array([code]), "msg": np.frombuffer(msg.encode(), dtype=np.uint8)}


JOBS = {"big_run": job_big_run, "capacity": job_capacity}


def child(job, env, tmp_path):
    out = os.path.join(str(tmp_path), job + "_" + "_".join(sorted(env)) + ".npz")
    e = dict(os.environ)
    for k in ("AMC_TEMP_RUN_UNFUSED", "AMC_TEMP_RUN_FUSED", "AMC_TEMP_UNFUSED", "AMC_STREAM_BS", "AMC_TEMP_DEV_CAP"):
        e.pop(k, None)
    e.update(env)
    r = subprocess.run([sys.executable, "-m", "tests.test_gpu_temp_run", job, out], cwd=ROOT, env=e, timeout=600,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def big():
    """The run (this process, default form) and the 20 single steps it has to equal."""
    run = job_big_run()
    eng, cfg, dt = big_engine()
    tot = dict.fromkeys(STAT_KEYS, 0)
    series, had, hits = [], [], dict.fromkeys(CASES, 0)
    for _ in range(BIG_STEPS):
        st, mom, cold, hot, hm, hc, hh = eng.temp_timestep_device(dt, cfg)
        for k in STAT_KEYS:
            tot[k] += st[k]
        series.append((mom, cold, hot))
        had.append((hm, hc, hh))
        for case in CASES:
            hits[case] += int(np.count_nonzero(eng.device_results(case)[3]))
    steps = snapshot(eng, tot, series, had)
    eng.close()
    return run, steps, hits


def test_run_equals_steps(big):
    """temp_run_device(dt, 20) == 20 x temp_timestep_device at N = 1e6: state, prior positions, summed counters, histograms,
    sorted path records, the 20 x 3 series and flags, and the last step's results / draws / sums."""
    run, steps, hits = big
    assert_same(run, steps, "run vs steps")
    assert all(hits[case] >= 1 for case in CASES), hits          # every case's sum is exercised ...
    assert sum(hits.values()) > 500 * BIG_STEPS // 3
    assert all(np.count_nonzero(run["series"][:, k]) > 0 for k in range(3))     # ... and all three series
    assert np.array_equal(run["series"][-1].view(np.uint64), run["last_sums"].view(np.uint64))
    assert np.array_equal(run["had"][-1], run["last_had"])


def test_fused_equals_unfused(big, tmp_path):
    """The same run with the single step's three streaming passes (AMC_TEMP_RUN_UNFUSED=1), and with the one fused pass asked
    for by name, in fresh processes: whichever is the default, both give the bits of the 20 single steps."""
    run, steps, _ = big
    assert_same(child("big_run", {"AMC_TEMP_RUN_UNFUSED": "1"}, tmp_path), steps, "unfused run vs steps")
    assert_same(child("big_run", {"AMC_TEMP_RUN_FUSED": "1"}, tmp_path), steps, "fused run vs steps")


def test_series_does_not_depend_on_the_order_of_the_records(big, tmp_path):
    """Other kernels append the hit records, in other atomic orders: the fused pass at another block size, and the per-case
    kernel triples behind the single step's passes.  The sums kernel orders the records itself."""
    run, steps, _ = big
    assert_same(child("big_run", {"AMC_TEMP_RUN_FUSED": "1", "AMC_STREAM_BS": "64"}, tmp_path), steps, "block size 64")
    assert_same(child("big_run", {"AMC_TEMP_RUN_UNFUSED": "1", "AMC_TEMP_UNFUSED": "1"}, tmp_path), steps, "per-case kernels")


def test_record_overflow_fails_the_run_and_names_the_case(tmp_path):
    got = child("capacity", {"AMC_TEMP_DEV_CAP": "8"}, tmp_path)
    msg = got["msg"].tobytes().decode()
    assert int(got["code"][0]) == -4, msg                           # AMC_ERR_CAPACITY
    assert "in case " in msg and "record capacity 8" in msg, msg


def test_arguments_are_checked_before_anything_runs():
    from argon_monte_carlo_amd._abi import AmcStepStats
    from argon_monte_carlo_amd.energised import device_rng_config
    from argon_monte_carlo_amd.engine import EnergisedEngine, Engine
    cfg = device_rng_config(PR.pore_params(n=2000, energised=True)[1], 5)
    p, c = PR.pore_params(n=2000)
    st = AmcStepStats()
    eng = Engine(p)
    eng.upload(*IC.pore_ic(p, c, seed=3))
    assert eng.lib.amc_temp_run_device(eng._ctx, c["dt"], 2, C.byref(cfg), C.byref(st)) == -6      # not an energised context
    eng.close()
    p, c = PR.pore_params(n=2000, energised=True)
    eng = EnergisedEngine(p)
    assert eng.lib.amc_temp_run_device(eng._ctx, c["dt"], 2, C.byref(cfg), C.byref(st)) == -6      # before amc_upload
    eng.upload(*IC.pore_ic(p, c, seed=3))
    assert eng.lib.amc_temp_run_device(eng._ctx, c["dt"], -1, C.byref(cfg), C.byref(st)) == -1
    assert eng.lib.amc_temp_run_device(eng._ctx, c["dt"], 2, None, C.byref(st)) == -1
    bad = device_rng_config(c, 5)
    bad.struct_size -= 8
    assert eng.lib.amc_temp_run_device(eng._ctx, c["dt"], 2, C.byref(bad), C.byref(st)) == -1
    assert eng.lib.amc_temp_series_read(eng._ctx, 0, 1, None, None, None) == -1                      # no run yet: no rows
    with pytest.raises(Exception) as ei:
        eng.run(c["dt"], 1)                                          # amc_run still refuses, and says where to go
    assert "amc_temp_run_device" in str(ei.value)
    st0, series, had = eng.temp_run_device(c["dt"], 0, cfg)          # an empty run is a run
    assert series.shape == (0, 3) and st0["n_wall"] == 0
    eng.close()


# ---- through TemperatureSimulation: a small system, where most steps have no energised hit -------------------------------
SMALL_N, SMALL_STEPS = 2000, 20     # about 1.2 energised hits per step (6e-4 per particle and step): see test_temp_run_host.py


def small_sim(monkeypatch):
    from argon_monte_carlo_amd.sim import TemperatureSimulation
    monkeypatch.setenv("AMC_GAP_WORKERS", "0")
    sim = TemperatureSimulation(n=SMALL_N, device_rng_seed=11)
    sim.init_synthetic(seed=23)
    return sim


def sim_results(sim, directory):
    os.makedirs(directory, exist_ok=True)
    sim.write_outputs(str(directory))
    with open(os.path.join(str(directory), "momentum_energy.csv"), "rb") as fh:
        csv = fh.read()
    st = sim.engine.download()
    return dict(mom=list(sim.momentum_z_change_per_step), cold=list(sim.energy_transfer_cold_per_step),
                hot=list(sim.energy_transfer_hot_per_step), zero=[tuple(z) for z in sim._zero_flags], cols=sim.total_cols,
                errs=sim.total_errs, done=sim.steps_done, csv=csv, state={k: st[k].tobytes() for k in STATE_KEYS})


def assert_sims_equal(a, b, what):
    for k in ("mom", "cold", "hot"):
        assert len(a[k]) == len(b[k]) and all(float(u).hex() == float(v).hex() for u, v in zip(a[k], b[k])), (what, k)
    for k in ("zero", "cols", "errs", "done", "csv", "state"):
        assert a[k] == b[k], (what, k)


@pytest.fixture()
def stepped(monkeypatch, tmp_path):
    sim = small_sim(monkeypatch)
    for _ in range(SMALL_STEPS):
        sim.timestep(collect_paths=False)
    res = sim_results(sim, tmp_path / "stepped")
    sim.close()
    return res


def test_simulation_run_equals_timesteps_with_and_without_hits(stepped, monkeypatch, tmp_path):
    sim = small_sim(monkeypatch)
    st = sim.run(SMALL_STEPS)
    res = sim_results(sim, tmp_path / "run")
    sim.close()
    assert st is not None and res["done"] == SMALL_STEPS
    assert_sims_equal(res, stepped, "run(k) vs k timesteps")
    none = [z == (True, True, True) for z in res["zero"]]
    assert any(none) and not all(none), res["zero"]                 # both kinds of step occurred
    rows = res["csv"].decode().splitlines()
    assert len(rows) == SMALL_STEPS + 1 and any(",0," in ("," + r + ",") for r in rows[1:])      # the literal 0 of a step without a hit


def test_simulation_run_in_segments_and_resumed(stepped, monkeypatch, tmp_path):
    sim = small_sim(monkeypatch)
    sim.run(7)
    ck = str(tmp_path / "after7.npz")
    sim.save_checkpoint(ck)
    sim.run(13)
    assert_sims_equal(sim_results(sim, tmp_path / "segments"), stepped, "run(7); run(13)")
    sim.close()
    sim = small_sim(monkeypatch)
    sim.load_checkpoint(ck)
    sim.run(13)
    assert_sims_equal(sim_results(sim, tmp_path / "resumed"), stepped, "checkpoint after 7, resumed for 13")
    sim.close()


def test_simulation_run_samples_fields_like_timesteps(monkeypatch):
    got = []
    for use_run in (False, True):
        sim = small_sim(monkeypatch)
        sim.enable_fields(every=5)
        if use_run:
            sim.run(SMALL_STEPS)
        else:
            for _ in range(SMALL_STEPS):
                sim.timestep(collect_paths=False)
        tot, ns, no = sim.engine.fields_read()
        got.append((tot.tobytes(), ns, no, sim.engine.download()["x"].tobytes()))
        sim.close()
    assert got[0][1] == SMALL_STEPS // 5
    assert got[0] == got[1]


if __name__ == "__main__":
    np.savez(sys.argv[2], **JOBS[sys.argv[1]]())
