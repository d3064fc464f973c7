"""GPU (-m gpu): the energised pore's seven wall cases (Temp:705-758) in all their forms against the oracle (`mul`) on the
crafted states of tests/edge_states.py — ``temp_walls()``: particles exactly on every plane and squared radius the masks
compare against, and at the corners where two cases hit one particle in one step; ``temp_many_hits()``: more hits in one step
than the device sums' tile holds.  The reference's own answer on these thresholds is tests/golden/func_temp_edge.npz, which
pins the oracle (tests/test_oracle_edges.py); here the bar is GPU == oracle, bit for bit.

The forms: the host hand-over case by case and as a whole step (with the gap case parked, and not), the device-draw single
step (one kernel for all cases, and AMC_TEMP_UNFUSED=1: a kernel triple per case), the host-free run (fused into the streaming
pass, and AMC_TEMP_RUN_UNFUSED=1), the device sums past their tile, the sampled surfaces.  The oracle replays a device-draw
step with the draws the device used (tests/test_gpu_draws.py pins the draws themselves, every hit against 40 digits).

Every test asserts on the ORACLE that the state did what it is there for (tests/edge_states.assert_temp_coverage): every case
hit, the corner sequences taken or blocked, a contact solve without a real root.

Runs that need other environment switches (read when a context is created) happen in fresh child processes, each under its
own time limit: ``python -m tests.test_gpu_temp_edges <job> <out.npz>``."""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from argon_monte_carlo_amd import params as PR  # noqa: E402
from argon_monte_carlo_amd import surface as SU  # noqa: E402
from argon_monte_carlo_amd.energised import CASES, COLD_CASES, GAP_CASE, HOT_CASES  # noqa: E402
from tests import edge_states as E  # noqa: E402
from tests import surface_ref as REF  # noqa: E402

pytestmark = pytest.mark.gpu

SF = ["x", "y", "z", "vx", "vy", "vz", "d", "dx", "dy", "dz"]
COUNTERS = ("n_pp", "n_wall", "n_oob_walls", "n_oob_pp", "n_paths", "n_fp_errors")
STAT_KEYS = COUNTERS + ("n_candidates",)
REC_KEYS = ("phase", "cell", "i", "j", "which", "total", "px", "py", "pz")
RNG_SEED = 0x5EED0EDCE5
STEPS = 4
SUMS_TILE, RECORD_CAP = 2048, 4096          # AMC_TEMP_SUMS_TILE; the record capacity per case at n < 196,608
_CACHE = {}


# ---- the states ------------------------------------------------------------------------------------------------------------------
def build(name):
    """(EdgeState with the params a context needs, constants, SurfaceEnergies) of "walls", "walls_slow", "many" or "failed"."""
    from argon_monte_carlo_amd.energised import SurfaceEnergies
    s = {"walls": E.temp_walls, "walls_slow": lambda: E.temp_walls(far=False), "many": E.temp_many_hits,
         "failed": E.temp_failed_only}[name]()
    c = PR.pore_params(n=s.n, energised=True)[1]
    if "energies" not in _CACHE:
        _CACHE["energies"] = SurfaceEnergies(c)
    en = _CACHE["energies"]
    s.p.reserved0 |= 1
    s.p.E_cold, s.p.E_hot = en.cold, en.hot          # Temp:83-84 (what the device uses for the coated walls)
    return s, c, en


def engine_of(s, grid=None):
    from argon_monte_carlo_amd.engine import EnergisedEngine
    eng = EnergisedEngine(s.p)
    a = s.arrays()
    eng.upload(*a[:10], flag=a[10])
    if grid is not None:
        eng.surface_config(grid)
    return eng


def oracle_of(s):
    from oracle import oracle as O
    orc = O.Oracle(s.p, mode="mul")
    a = s.arrays()
    orc.upload(*a[:10], flag=a[10])
    return orc


def samplers():
    from argon_monte_carlo_amd.energised import DirectionSampler
    return (DirectionSampler(np.random.RandomState(17), random.Random(17)),
            DirectionSampler(np.random.RandomState(17), random.Random(17)))


@pytest.fixture(scope="module", autouse=True)
def cpu_first():
    """Every state through the oracle on the CPU (its own host loop, host draws) before any of it goes to the GPU: finite."""
    for name, steps in (("walls", STEPS), ("walls_slow", STEPS), ("many", 1), ("failed", 2)):
        s, c, en = build(name)
        orc = oracle_of(s)
        smp = samplers()[0]
        for q in range(steps):
            rc, *_ = orc.temp_timestep(s.dt, smp, en)
            assert rc == 0, (name, q)
            st = orc.state()
            for k in SF:
                assert np.isfinite(st[k]).all(), (name, q, k)
        r = orc.paths()
        for k in ("total", "px", "py", "pz"):
            assert np.isfinite(r[k]).all(), (name, k)


# ---- comparing ------------------------------------------------------------------------------------------------------------------
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same(a, b, ctx):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (ctx, a.shape, b.shape)
    assert np.array_equal(bits(a), bits(b)), (ctx, np.flatnonzero(np.ravel(bits(a) != bits(b)))[:5])


def assert_state_equal(dev, orc, ctx, skip_velocity=()):
    keep = np.ones(len(dev["x"]), dtype=bool)
    keep[list(skip_velocity)] = False
    for k in SF:
        m = keep if k in ("vx", "vy", "vz") else slice(None)
        assert np.array_equal(dev[k][m], orc[k][m]), (ctx, k, np.flatnonzero(dev[k] != orc[k])[:5])
    assert np.array_equal(dev["flag"].astype(bool), orc["flag"].astype(bool)), (ctx, "flag")


def canonical(r):
    return r[np.lexsort((r["pz"], r["py"], r["px"], r["total"], r["which"], r["j"], r["i"], r["cell"], r["phase"]))]


def assert_records_equal(dev, orc, ctx):
    d, o = canonical(dev), canonical(orc)
    assert len(d) == len(o), (ctx, len(d), len(o))
    for k in REC_KEYS:
        assert np.array_equal(d[k], o[k]), (ctx, k)


def assert_same(a, b, what):
    assert sorted(a) == sorted(b), what
    for k in sorted(a):
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, (what, k, a[k].shape, b[k].shape)
        assert np.array_equal(bits(a[k]), bits(b[k])), (what, k)


# ---- the oracle's half of a step -------------------------------------------------------------------------------------------------
def orc_begin(orc, dt):
    orc._temp_wall_count = orc._temp_errs = 0
    orc._paths_before = orc._sink.n
    orc.drift(dt, True)                                 # Temp:672-683
    orc._temp_errs += orc.temp_specular()               # Temp:693-703


def orc_end(orc):
    oob1 = orc.bounds(True)                             # Temp:804
    rc, npp, _ = orc.sweep()                            # Temp:813-842
    oob2 = orc.bounds(True)                             # Temp:844
    orc.step += 1
    assert rc == 0
    return dict(n_pp=npp, n_wall=orc._temp_wall_count, n_oob_walls=oob1, n_oob_pp=oob2, n_paths=orc._sink.n - orc._paths_before,
                n_fp_errors=orc._temp_errs)


def orc_contacts(orc, n):
    return orc._pending[4][:n].copy()


class Coverage:
    """the first step's hits per case and failed solves, as the oracle saw them"""

    def __init__(self):
        self.masks, self.failed = {}, 0

    def note(self, case, idx, ok):
        if case not in self.masks:
            self.masks[case] = np.array(idx)
            self.failed += int(np.count_nonzero(~np.asarray(ok)))

    def spy(self, orc):
        orig = orc.wall_hits

        def wall_hits(case):
            r = orig(case)
            self.note(case, r[0], r[3])
            return r
        orc.wall_hits = wall_hits
        return self

    def check(self, s):
        E.assert_temp_coverage(s, self.masks, self.failed)


# ---- 1. the host hand-over, case by case -----------------------------------------------------------------------------------------
def chosen_directions(normals, ok):
    """A unit vector per hit, 37 degrees off the inward normal (0.8 n + 0.6 t, t a unit vector across n that turns from hit
    to hit): well outside the grazing band of Temp:136."""
    d = np.zeros((len(normals), 3))
    for k, (n, good) in enumerate(zip(normals, ok)):
        if not good:
            continue
        a = 0.3 + 0.7 * k
        t = np.array([np.cos(a), np.sin(a), 0.0]) if n[2] != 0.0 else np.array([-n[1] * np.cos(a), n[0] * np.cos(a), np.sin(a)])
        d[k] = 0.8 * n + 0.6 * t
    return d


def chosen_energies(case, ok, en):
    Es = np.zeros(len(ok))
    Es[np.asarray(ok)] = 1.25 * en.hot if case == GAP_CASE else (en.cold if case in COLD_CASES else en.hot)
    return Es


@pytest.mark.parametrize("park", [False, True])
def test_hand_over_case_by_case(park):
    """temp_begin; per case wall_hits -> wall_contacts -> wall_apply with directions and energies the test chooses; temp_end:
    indices, normals, contact points, solve flags, dp_z, dE and the full state after EVERY case, counters and path records at
    the end.  park: the gap case is parked (wall_park) and finished (wall_finish) when a later case hits a parked particle —
    the corner particles make case 6 do so — with wall_hits_again, as drive_energised_cases does."""
    s, c, en = build("walls")
    eng, orc = engine_of(s), oracle_of(s)
    cov = Coverage()
    eng.temp_begin(s.dt)
    orc_begin(orc, s.dt)
    parked, again = None, 0

    def finish():
        idx5, Es5, want = parked
        dpz, dE = eng.wall_finish(GAP_CASE, Es5)
        same(dpz, want[0], "parked dpz")
        same(dE, want[1], "parked dE")

    for case in CASES:
        idx, nm, cz, ok = eng.wall_hits(case)
        if parked is not None and np.intersect1d(parked[0], idx).size:
            finish()
            parked, again = None, again + 1
            eng.wall_hits_again()
            idx, nm, cz, ok = eng.wall_hits(case)
        xyz = eng.wall_contacts(case, len(idx))
        oidx, onm, ocz, ook = orc.wall_hits(case)
        cov.note(case, oidx, ook)
        same(idx, oidx, (case, "idx"))
        same(nm, onm, (case, "normals"))
        same(cz, ocz, (case, "contact z"))
        same(ok, ook, (case, "ok"))
        same(xyz, orc_contacts(orc, len(oidx)), (case, "contacts"))
        assert len(idx) > 0, case
        dirs, Es = chosen_directions(onm, ook), chosen_energies(case, ook, en)
        want = orc.wall_apply(case, dirs, Es)
        if park and case == GAP_CASE:
            eng.wall_park(case, dirs)
            parked = (idx, Es, want)
        else:
            dpz, dE = eng.wall_apply(case, dirs, Es)
            same(dpz, want[0], (case, "dpz"))
            same(dE, want[1], (case, "dE"))
        assert_state_equal(eng.download(), orc.state(), (park, case), skip_velocity=() if parked is None else parked[0])
    if parked is not None:
        finish()
    st, so = eng.temp_end(), orc_end(orc)
    for k in COUNTERS:
        assert st[k] == so[k], (k, st, so)
    assert_state_equal(eng.download(), orc.state(), (park, "end"))
    assert_records_equal(eng.drain_paths(sort=True), orc.paths(), park)
    cov.check(s)
    assert again == (1 if park else 0)
    eng.close()


# ---- 2. the host hand-over, whole steps ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("park", [True, False])
def test_hand_over_whole_steps(monkeypatch, park):
    """temp_timestep with a DirectionSampler and SurfaceEnergies on both sides, 3 steps; with parking (the default: the
    finish-first path runs because case 6 hits parked corner particles, nothing forces it) and with AMC_TEMP_NO_PARK=1."""
    monkeypatch.setenv("AMC_GAP_WORKERS", "0")
    monkeypatch.delenv("AMC_TEMP_FORCE_GAP_REDO", raising=False)
    if park:
        monkeypatch.delenv("AMC_TEMP_NO_PARK", raising=False)
    else:
        monkeypatch.setenv("AMC_TEMP_NO_PARK", "1")
    s, c, en = build("walls")
    eng, orc = engine_of(s), oracle_of(s)
    cov = Coverage().spy(orc)
    calls = {"wall_park": 0, "wall_hits_again": 0}

    def counted(name):
        orig = getattr(eng, name)

        def call(*a):
            calls[name] += 1
            return orig(*a)
        setattr(eng, name, call)
    for name in calls:
        counted(name)
    s_dev, s_orc = samplers()
    for q in range(3):
        st, *dev = eng.temp_timestep(s.dt, s_dev, en)
        rc, so, *ref = orc.temp_timestep(s.dt, s_orc, en)
        assert rc == 0
        for k in COUNTERS:
            assert st[k] == so[k], (q, k, st, so)
        assert tuple(dev) == tuple(ref), (q, dev, ref)
        assert_state_equal(eng.download(), orc.state(), (park, q))
    assert_records_equal(eng.drain_paths(sort=True), orc.paths(), park)
    cov.check(s)
    assert min(calls.values()) >= 1 if park else max(calls.values()) == 0, calls
    eng.close()


# ---- jobs: device draws (this process, or a child with another environment) ----------------------------------------------------
def snapshot(eng, stats, series, had):
    out = {f"state_{k}": v for k, v in eng.download().items()}
    out["prior"] = np.stack(eng.download_prior())
    out["stats"] = np.array([stats[k] for k in STAT_KEYS], dtype=np.int64)
    counts, tot = eng.histograms()
    out["hist"], out["hist_total"] = counts, np.array([tot], dtype=np.uint64)
    out["paths"] = np.frombuffer(eng.drain_paths(sort=True).tobytes(), dtype=np.uint8)
    out["series"], out["had"] = np.asarray(series, dtype=np.float64).reshape(-1, 3), np.asarray(had, dtype=bool).reshape(-1, 3)
    for case in CASES:
        for name, arrs in (("res", eng.device_results(case)), ("draw", eng.device_draws(case))):
            for k, a in enumerate(arrs):
                out[f"{name}_{case}_{k}"] = np.asarray(a)
    sums, hd = (C.c_double * 3)(), (C.c_int32 * 3)()
    eng._ck(eng.lib.amc_temp_device_sums(eng._ctx, sums, hd))
    out["last_sums"], out["last_had"] = np.array(list(sums)), np.array([bool(v) for v in hd])
    return out


def job_steps(name, nsteps, surfaces=False):
    """nsteps single device-draw steps: per step t and case k the draws, results and contacts ("t<t>_..."), the state and the
    counters; at the end the snapshot a run of nsteps has to equal ("end_...")."""
    from argon_monte_carlo_amd.energised import device_rng_config
    s, c, en = build(name)
    eng = engine_of(s, SU.default_grid(s.p) if surfaces else None)
    cfg = device_rng_config(c, RNG_SEED)
    out, tot, series, had = {}, dict.fromkeys(STAT_KEYS, 0), [], []
    for t in range(nsteps):
        st, mom, cold, hot, hm, hc, hh = eng.temp_timestep_device(s.dt, cfg)
        series.append((mom, cold, hot))
        had.append((hm, hc, hh))
        for k in STAT_KEYS:
            tot[k] += st[k]
        out[f"t{t}_stats"] = np.array([st[k] for k in STAT_KEYS], dtype=np.int64)
        for case in CASES:
            for kind, arrs in (("draw", eng.device_draws(case)), ("res", eng.device_results(case)), ("con", eng.device_contacts(case))):
                for k, a in enumerate(arrs):
                    out[f"t{t}_{kind}_{case}_{k}"] = np.asarray(a)
        for k, v in eng.download().items():
            out[f"t{t}_state_{k}"] = v
        if surfaces:
            tt, nf, ns = eng.surface_read()
            out[f"t{t}_surf_totals"], out[f"t{t}_surf_failed"], out[f"t{t}_surf_steps"] = tt, nf, np.array([ns])
    out.update({"end_" + k: v for k, v in snapshot(eng, tot, series, had).items()})
    eng.close()
    return out


def job_run(name, nsteps):
    from argon_monte_carlo_amd.energised import device_rng_config
    s, c, en = build(name)
    eng = engine_of(s)
    st, series, had = eng.temp_run_device(s.dt, nsteps, device_rng_config(c, RNG_SEED))
    out = {"end_" + k: v for k, v in snapshot(eng, st, series, had).items()}
    eng.close()
    return out


JOBS = {"steps_walls": lambda: job_steps("walls", STEPS), "run_walls": lambda: job_run("walls", STEPS),
        "steps_many": lambda: job_steps("many", 1), "run_many": lambda: job_run("many", 1)}


def child(job, env, tmp_path):
    out = os.path.join(str(tmp_path), job + "_" + "_".join(sorted(env)) + ".npz")
    e = dict(os.environ)
    for k in ("AMC_TEMP_RUN_UNFUSED", "AMC_TEMP_RUN_FUSED", "AMC_TEMP_UNFUSED", "AMC_STREAM_BS", "AMC_TEMP_DEV_CAP", "AMC_TEMP_NO_PARK"):
        e.pop(k, None)
    e.update(env)
    r = subprocess.run([sys.executable, "-m", "tests.test_gpu_temp_edges", job, out], cwd=ROOT, env=e, timeout=120,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


def end_of(d):
    return {k[4:]: v for k, v in d.items() if k.startswith("end_")}


@pytest.fixture(scope="module")
def steps_walls():
    return JOBS["steps_walls"]()


@pytest.fixture(scope="module")
def steps_many():
    return JOBS["steps_many"]()


# ---- 3. device draws, single steps -----------------------------------------------------------------------------------------------
def replay(s, D, nsteps):
    """The oracle through nsteps steps with the draws the device used (D: a job_steps dump): hits, normals, contact points,
    solve flags, dp_z, dE per case, the state and the counters per step, the path records at the end.  Returns the oracle,
    its first step's coverage and per step the records (case, contact, ok, dpz, dE, particle) in case and index order."""
    orc = oracle_of(s)
    cov, records = Coverage(), []
    for t in range(nsteps):
        orc_begin(orc, s.dt)
        recs = []
        for case in CASES:
            idx, nm, cz, ok = orc.wall_hits(case)
            xyz = orc_contacts(orc, len(idx))
            cov.note(case, idx, ok)
            didx, dn, dcz, ddir, dEs = (D[f"t{t}_draw_{case}_{k}"] for k in range(5))
            same(didx, idx, (t, case, "idx"))
            same(dn, nm, (t, case, "normals"))
            same(dcz, cz, (t, case, "contact z"))
            dpz, dE = orc.wall_apply(case, ddir, dEs)
            ridx, rdpz, rdE, rok = (D[f"t{t}_res_{case}_{k}"] for k in range(4))
            same(ridx, idx, (t, case, "result idx"))
            same(rok, ok, (t, case, "ok"))
            same(rdpz, dpz, (t, case, "dpz"))
            same(rdE, dE, (t, case, "dE"))
            same(D[f"t{t}_con_{case}_0"], idx, (t, case, "contact idx"))
            same(D[f"t{t}_con_{case}_1"], xyz, (t, case, "contacts"))
            recs += [(case, tuple(xyz[k]), bool(ok[k]), float(dpz[k]), float(dE[k]), int(idx[k])) for k in range(len(idx))]
        so = orc_end(orc)
        st = dict(zip(STAT_KEYS, D[f"t{t}_stats"].tolist()))
        for k in COUNTERS:
            assert st[k] == so[k], (t, k, st, so)
        assert_state_equal({k: D[f"t{t}_state_{k}"] for k in SF + ["flag"]}, orc.state(), t)
        records.append(recs)
    return orc, cov, records


def path_records(raw):
    from argon_monte_carlo_amd._abi import path_record_dtype
    return np.frombuffer(raw.tobytes(), dtype=path_record_dtype())


@pytest.mark.parametrize("unfused", [False, True])
def test_device_draw_steps_match_oracle(steps_walls, tmp_path, unfused):
    """temp_timestep_device, 4 steps, in its default form (k_temp_all) and with AMC_TEMP_UNFUSED=1 (k_temp_hits / k_temp_sample /
    k_temp_apply per case, a fresh process): every multi-case particle has its masks re-evaluated after the previous case moved
    it."""
    D = child("steps_walls", {"AMC_TEMP_UNFUSED": "1"}, tmp_path) if unfused else steps_walls
    s = build("walls")[0]
    orc, cov, _ = replay(s, D, STEPS)
    cov.check(s)
    assert_records_equal(path_records(D["end_paths"]), orc.paths(), unfused)
    if unfused:
        assert_same(D, steps_walls, "per-case kernels vs one kernel")


# ---- 4. the run forms ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["default", "AMC_TEMP_RUN_UNFUSED", "AMC_TEMP_RUN_FUSED"])
def test_run_forms_equal_single_steps(steps_walls, tmp_path, form):
    """temp_run_device(dt, 4) == 4 single steps on temp_walls(): state, prior positions, counters, histograms, sorted records,
    the series and flags, the last step's results, draws and sums — the stage fused into the streaming pass carries px, py,
    pz in registers through the case sequence."""
    s = build("walls")[0]
    _, cov, _ = replay(s, steps_walls, 1)
    cov.check(s)
    run = JOBS["run_walls"]() if form == "default" else child("run_walls", {form: "1"}, tmp_path)
    assert_same(end_of(run), end_of(steps_walls), form)
    assert np.count_nonzero(end_of(run)["had"]) >= 3


# ---- 5. the device sums past their tile --------------------------------------------------------------------------------------
def python_sums(records):
    """(sums[3], had[3]) of one step from per-hit records in case and ascending particle order: per case left to right from
    0.0, failed solves skipped; the cases folded in order 3 .. 9 (a case without a hit adds nothing)."""
    sums, had = [0.0, 0.0, 0.0], [False, False, False]
    for case in CASES:
        mine = [r for r in records if r[0] == case]
        if not mine:
            continue
        assert [r[5] for r in mine] == sorted(r[5] for r in mine)
        m_case, e_case, good = 0.0, 0.0, False
        for _, _, ok, dpz, dE, _ in mine:
            if ok:
                m_case, e_case, good = m_case + dpz, e_case + dE, True
        sums[0] = sums[0] + m_case
        had[0] = had[0] or good
        if case in COLD_CASES:
            sums[1], had[1] = sums[1] + e_case, had[1] or good
        elif case in HOT_CASES:
            sums[2], had[2] = sums[2] + e_case, had[2] or good
    return np.array(sums), np.array(had)


def test_sums_past_the_tile(steps_many, tmp_path):
    """temp_many_hits(): more than 2048 hits in one step, so k_case_sums ranks and permutes through global memory; some of
    case 8's solves fail and are skipped.  The single step's sums, the run's series row and amc_temp_device_sums equal the
    left-to-right Python sum of the oracle's per-hit values; unchanged with AMC_STREAM_BS=64 (another atomic order)."""
    s = build("many")[0]
    _, cov, records = replay(s, steps_many, 1)
    recs = records[0]
    per_case = {case: sum(1 for r in recs if r[0] == case) for case in CASES}
    assert sum(per_case.values()) > SUMS_TILE and max(per_case.values()) < RECORD_CAP, per_case
    assert sum(1 for v in per_case.values() if v > 0) >= 3, per_case
    assert [r[5] for r in recs if r[0] == 3] != list(range(per_case[3]))          # (indices interleaved over the cases)
    ok8 = [r[2] for r in recs if r[0] == 8]
    assert any(ok8) and not all(ok8), (len(ok8), sum(ok8))          # a case in which some solves fail and some do not
    ok9 = [r[2] for r in recs if r[0] == 9]
    assert len(ok9) == 5 and not any(ok9)                           # and one whose every hit is a failed solve
    want, want_had = python_sums(recs)
    assert np.all(want != 0.0) and want_had.all()
    single = end_of(steps_many)
    run = end_of(JOBS["run_many"]())
    bs64 = end_of(child("run_many", {"AMC_STREAM_BS": "64"}, tmp_path))
    for what, got in (("single step", single), ("run", run), ("block size 64", bs64)):
        same(got["series"][0], want, (what, "series row"))
        same(got["last_sums"], want, (what, "amc_temp_device_sums"))
        same(got["had"][0], want_had, (what, "had"))
        same(got["last_had"], want_had, (what, "last had"))
    assert_same(run, single, "run vs single step")
    assert_same(bs64, single, "block size 64 vs single step")


def test_sums_skip_failed_solves_and_clear_had(steps_walls):
    """On temp_walls() (the tiled branch): per step the sums and flags equal the Python sum over the oracle's records; a sum
    whose cases had hits but only failed solves, or no hit, has its flag clear."""
    s = build("walls")[0]
    _, cov, records = replay(s, steps_walls, STEPS)
    cov.check(s)
    end = end_of(steps_walls)
    for t, recs in enumerate(records):
        want, want_had = python_sums(recs)
        same(end["series"][t], want, (t, "series"))
        same(end["had"][t], want_had, (t, "had"))
    assert any(not r[2] for r in records[0])


def test_a_sum_of_failed_solves_only_keeps_its_flag_clear():
    """temp_failed_only(): in step 0 the hot sum's only hits (case 8) are failed solves, the cold sum has good hits (case 3)
    and failed ones (case 9); in step 1 every hit of the step is a failed solve.  A case with records but no good hit folds
    + 0.0 into its sums and leaves their flags clear — in the single step and in the run."""
    s = build("failed")[0]
    D = job_steps("failed", 2)
    _, _, records = replay(s, D, 2)
    for case, n_hits, n_ok in ((3, 5, 5), (8, 5, 0), (9, 5, 0)):
        mine = [r[2] for r in records[0] if r[0] == case]
        assert (len(mine), sum(mine)) == (n_hits, n_ok), (case, mine)
    assert len(records[1]) >= 5 and not any(r[2] for r in records[1])
    single, run = end_of(D), end_of(job_run("failed", 2))
    for t, flags in enumerate(((True, True, False), (False, False, False))):
        want, want_had = python_sums(records[t])
        assert tuple(want_had) == flags and want[2] == 0.0, (t, want, want_had)
        for what, got in (("single steps", single), ("run", run)):
            same(got["series"][t], want, (what, t, "series"))
            same(got["had"][t], want_had, (what, t, "had"))
    same(single["last_had"], np.array([False, False, False]), "amc_temp_device_sums")
    assert_same(run, single, "run vs single steps")


# ---- 6. the sampled surfaces -----------------------------------------------------------------------------------------------------
def test_surfaces_on_the_edges():
    """temp_walls(far=False) with the default surface grid, 3 device-draw steps: the integer totals and the failed-solve
    counts equal tests/surface_ref applied to the ORACLE's hit records.  The contacts of cases 8 and 9 after a plane case
    sit exactly on t_z3_hot, t_zgap_lo, t_zgap_hi: the range ends of the cylinder surfaces."""
    D = job_steps("walls_slow", 3, surfaces=True)
    s = build("walls_slow")[0]
    _, cov, records = replay(s, D, 3)
    cov.check(s)
    g = SU.default_grid(s.p)
    nb, lo, hi = int(g.nbins), list(g.lo), list(g.hi)
    tot, failed = REF.empty(nb)
    on_end = 0
    for t, recs in enumerate(records):
        REF.accumulate(tot, failed, nb, lo, hi, recs)
        same(D[f"t{t}_surf_totals"], REF.to_words(tot), (t, "totals"))
        assert D[f"t{t}_surf_failed"].tolist() == failed and int(D[f"t{t}_surf_steps"][0]) == t + 1, (t, failed)
        on_end += sum(1 for case, xyz, ok, *_ in recs if ok and case in (8, 9) and xyz[2] in (lo[case - 3], hi[case - 3]))
    assert sum(failed) >= 1 and on_end >= 1, (failed, on_end)


if __name__ == "__main__":
    np.savez(sys.argv[2], **JOBS[sys.argv[1]]())
