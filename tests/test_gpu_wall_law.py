"""GPU (-m gpu): the Maxwell wall law of the device-RNG energised pore (include/argonmc-walllaw.h, DESIGN.md 21;
csrc/amc_energised_dev.h: temp_maxwell_draw, temp_maxwell_finish) against references that are not the device's own numbers
(tests/wall_law_ref.py): the recipe with mpmath at 40 digits, which also takes the diffuse / specular decisions.

The state is edge_states.temp_draw_hits(): N = 1,330, every particle a hit in its first step, 190 per case.  It is uploaded
afresh and stepped once per step word of tests/test_wall_law_host.py: step 0 and one step per entry of its table (the smallest
and the largest ua and ub, u0 on either side of either alpha, step words up to 0x3fffffff, the largest amc_set_step admits) at
alpha_coated = 0.95, alpha_gap = 0.8.

Tolerance: velocity components within 16 * MIRROR_VEL_ERR * s of the reference, s = sqrt(k T_w / m) of the hit —
MIRROR_VEL_ERR is what the float64 mirror measures against the 40-digit reference (test_wall_law_host.py prints it and holds it
under the literal), 16 the factor of tests/test_gpu_draws.py for a device libm that rounds otherwise.  Everything else is bit
for bit: the decisions (read from Es), Es itself, dp_z, dE and dir recomputed from the device's own new velocity, the position,
the accumulators.

Eight particles (draw_corner_4_8) are hit twice in the step, by case 4 and then by case 8.  The velocity between their two hits
is nowhere to be read, so: their first hit's records are compared only when the second contact solve failed; a specular
second hit is compared with the reference fed the reference's first-hit velocity, at (1 + sqrt 3) times the tolerance (a
reflection is an isometry: a component moves by at most the Euclidean norm of the first hit's error); and since their second
contact solve sees a law-dependent velocity, their paths and failed solves are left out of the comparison with the reference
law's counters and paths.

The forms: the single step (k_temp_all<MAXWELL>), AMC_TEMP_UNFUSED=1 (k_temp_maxwell), the host-free run of one step after
set_step (k_stream<ENERGISED, 2>) and AMC_TEMP_RUN_UNFUSED=1.  The first is compared with the references; the other three must
return its draws, results, contacts, states and counters bit for bit on every step word.  Forms that need an environment switch
run in fresh child processes, each under its own time limit: ``python -m tests.test_gpu_wall_law <job> <out.npz>``."""
import math
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch                # (first: the library then shares torch's HIP runtime — LocalRanks exchanges through torch)  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from argon_monte_carlo_amd import ic as IC  # noqa: E402
from argon_monte_carlo_amd import params as PR  # noqa: E402
from argon_monte_carlo_amd.energised import CASES  # noqa: E402
from tests import draw_ref as R  # noqa: E402
from tests import surface_ref as SREF  # noqa: E402
from tests import test_draws_host as DH  # noqa: E402
from tests import test_wall_law_host as H  # noqa: E402
from tests import wall_law_ref as W  # noqa: E402

pytestmark = pytest.mark.gpu

SEED, STEPS, AC, AG = H.SEED, H.STEPS, H.ALPHA_COATED, H.ALPHA_GAP
VEL_RTOL = 16 * H.MIRROR_VEL_ERR
assert VEL_RTOL <= 1e-13
MAXWELL = 1
SF = ["x", "y", "z", "vx", "vy", "vz", "d", "dx", "dy", "dz"]
STAT_KEYS = ("n_pp", "n_wall", "n_oob_walls", "n_oob_pp", "n_paths", "n_fp_errors", "n_candidates")
SWITCHES = ("AMC_TEMP_RUN_UNFUSED", "AMC_TEMP_RUN_FUSED", "AMC_TEMP_UNFUSED", "AMC_STREAM_BS", "AMC_TEMP_DEV_CAP", "AMC_TEMP_NO_PARK")


# ---- jobs (this process, or a child with another environment) ----------------------------------------------------------------
def engine_of(s):
    from argon_monte_carlo_amd.engine import EnergisedEngine
    return EnergisedEngine(s.p)


def fresh(eng, s, step):
    a = s.arrays()
    eng.upload(*a[:10], flag=a[10])
    eng.reset_outputs()
    eng.set_step(step)


def dump(eng, out, tag, stats):
    out[f"{tag}_stats"] = np.array([stats[k] for k in STAT_KEYS], dtype=np.int64)
    for case in CASES:
        for kind, arrs in (("draw", eng.device_draws(case)), ("res", eng.device_results(case)), ("con", eng.device_contacts(case))):
            for k, a in enumerate(arrs):
                out[f"{tag}_{kind}_{case}_{k}"] = np.asarray(a)
    for k, v in eng.download().items():
        out[f"{tag}_state_{k}"] = v
    out[f"{tag}_paths"] = np.frombuffer(eng.drain_paths(sort=True).tobytes(), dtype=np.uint8)


def job(run, law=(MAXWELL, AC, AG), steps=STEPS, back=False):
    """The state uploaded afresh and taken through ONE step per step word under ``law`` (None: never set), as a single step
    (run=False) or as a host-free run of one step.  ``back``: every step word is first stepped under the Maxwell law, then the
    law is taken back (wall_law(None)), the state uploaded again and stepped: what is dumped is that second step."""
    from argon_monte_carlo_amd.energised import device_rng_config
    s, c, en = DH.state()
    cfg = device_rng_config(c, SEED)
    eng = engine_of(s)
    out = {}

    def one(step):
        fresh(eng, s, step)
        return eng.temp_run_device(s.dt, 1, cfg)[0] if run else eng.temp_timestep_device(s.dt, cfg)[0]
    if law is not None and not back:
        eng.wall_law(*law)
        assert eng.wall_law_get() == tuple(law)
    for i, step in enumerate(steps):
        if back:
            eng.wall_law(MAXWELL, AC, AG)
            one(step)
            eng.wall_law(None)
        st = one(step)
        dump(eng, out, f"s{i}", st)
    eng.close()
    return out


FEW = STEPS[:3]
JOBS = {"steps": lambda: job(False), "run": lambda: job(True), "default": lambda: job(False, law=None),
        "back": lambda: job(False, back=True), "alpha0": lambda: job(False, law=(MAXWELL, 0.0, 0.0), steps=FEW),
        "alpha1": lambda: job(False, law=(MAXWELL, 1.0, 1.0), steps=FEW)}


def child(name, env, tmp_path):
    out = os.path.join(str(tmp_path), name + "_" + "_".join(sorted(env)) + ".npz")
    e = dict(os.environ)
    for k in SWITCHES:
        e.pop(k, None)
    e.update(env)
    r = subprocess.run([sys.executable, "-m", "tests.test_gpu_wall_law", name, out], cwd=ROOT, env=e, timeout=120,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def steps():
    return JOBS["steps"]()


@pytest.fixture(scope="module")
def default():
    return JOBS["default"]()


# ---- comparing ------------------------------------------------------------------------------------------------------------------
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same(a, b, ctx):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (ctx, a.shape, b.shape)
    assert np.array_equal(bits(a), bits(b)), (ctx, np.flatnonzero(np.ravel(bits(a) != bits(b)))[:5])


def assert_same(a, b, what):
    assert sorted(a) == sorted(b), what
    for k in sorted(a):
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, (what, k, a[k].shape, b[k].shape)
        assert np.array_equal(bits(a[k]), bits(b[k])), (what, k)


def hits_of(D, i):
    """the hits of step word i in the order the device took them (case by case, ascending particle index inside a case): list
    of dicts with case, particle, ok, normal, contact, dir, Es, dpz, dE, and ``nth`` / ``of``: which ok hit of its particle"""
    out = []
    for case in CASES:
        idx, nm, cz, dirs, Es = (D[f"s{i}_draw_{case}_{k}"] for k in range(5))
        ridx, dpz, dE, ok = (D[f"s{i}_res_{case}_{k}"] for k in range(4))
        cidx, xyz = D[f"s{i}_con_{case}_0"], D[f"s{i}_con_{case}_1"]
        assert np.array_equal(idx, ridx) and np.array_equal(idx, cidx) and np.all(np.diff(idx) > 0), (i, case)
        assert np.array_equal(cz, xyz[:, 2]), (i, case)
        for k in range(len(idx)):
            out.append(dict(case=case, p=int(idx[k]), ok=bool(ok[k]), normal=nm[k], contact=xyz[k], dir=dirs[k], Es=float(Es[k]),
                            dpz=float(dpz[k]), dE=float(dE[k])))
    count = {}
    for h in out:
        if h["ok"]:
            h["nth"] = count[h["p"]] = count.get(h["p"], 0) + 1
    for h in out:
        if h["ok"]:
            h["of"] = count[h["p"]]
    return out


def law_consts():
    s, c, en = DH.state()
    return s, R.gap_consts(c), float(s.p.argon_mass)


def ref_of(step, h, v_in, alphas=(AC, AG)):
    s, g, m = law_consts()
    key = ("wl", step, h["case"], h["p"], h["normal"].tobytes(), h["contact"].tobytes(), np.asarray(v_in).tobytes(), alphas)
    if key not in DH._CACHE:
        DH._CACHE[key] = W.reference(SEED, [h["p"]], step, h["case"], h["normal"], h["contact"][2], v_in, alphas[0], alphas[1], g, m)
    return DH._CACHE[key]


def mirror_of(step, h, v_in, alphas=(AC, AG)):
    s, g, m = law_consts()
    return W.mirror(SEED, [h["p"]], step, h["case"], h["normal"], h["contact"][2], v_in, alphas[0], alphas[1], g, m)


# ---- 1. the single step against the 40-digit reference --------------------------------------------------------------------------
def test_single_step_is_the_40_digit_references(steps, capsys):
    """Every hit of every step word: the decision, Es, the new velocity, the records, the position and the accumulators."""
    s, g, m = law_consts()
    v0 = np.stack([s.vx, s.vy, s.vz], axis=1)
    corners = set(int(p) for p in s.cases["draw_corner_4_8"])
    worst, n_hits, n_diffuse, n_specular, n_chained, n_records = 0.0, 0, 0, 0, 0, 0
    for i, step in enumerate(STEPS):
        state = {k: steps[f"s{i}_state_{k}"] for k in SF}
        vel = np.stack([state["vx"], state["vy"], state["vz"]], axis=1)
        first_ref = {}
        for h in hits_of(steps, i):
            if not h["ok"]:
                assert not h["dir"].any() and h["Es"] == 0.0 and h["dpz"] == 0.0 and h["dE"] == 0.0, (hex(step), h["p"])
                continue
            p, last, chained = h["p"], h["nth"] == h["of"], h["nth"] > 1
            assert h["of"] == 1 or p in corners, (hex(step), p)
            mir = mirror_of(step, h, v0[p])
            diffuse = bool(mir["diffuse"][0])
            # the decision (an exact comparison of two doubles) and Es (plain arithmetic) are the mirror's, bit for bit
            assert (h["Es"] != 0.0) == diffuse and h["Es"] == float(mir["Es"][0]), (hex(step), h["case"], p, h["Es"])
            n_hits, n_diffuse, n_specular = n_hits + 1, n_diffuse + diffuse, n_specular + (not diffuse)
            v_in = first_ref[p] if chained else v0[p]
            ref = ref_of(step, h, v_in)
            assert bool(ref["diffuse"][0]) == diffuse and ref["margin"][0] > 0.0
            if not chained:
                first_ref[p] = ref["w"][0]
            if last:
                tol = VEL_RTOL * ref["s"][0]
                if chained and not diffuse:
                    tol *= 1.0 + math.sqrt(3.0)
                    n_chained += 1
                err = np.abs((vel[p] - ref["w"][0]) - ref["w_lo"][0])
                worst = max(worst, float(err.max() / ref["s"][0]))
                assert err.max() <= tol, (hex(step), h["case"], p, diffuse, float(err.max() / ref["s"][0]))
                # the particle stands on the contact point with empty accumulators (a second hit's contact comes from a drawn
                # velocity and may lie outside the domain, where the bounds check moves the particle: not asked of those)
                assert chained or [state["x"][p], state["y"][p], state["z"][p]] == h["contact"].tolist(), (hex(step), p)
                assert state["d"][p] == state["dx"][p] == state["dy"][p] == state["dz"][p] == 0.0, (hex(step), p)
            if last and not chained:
                # the records from the device's own new velocity, bit for bit
                d, dpz, dE = W.finish(v0[p][None, :], vel[p][None, :], m)
                same(h["dir"], d[0], (hex(step), h["case"], p, "dir"))
                same(np.float64(h["dpz"]), dpz[0], (hex(step), h["case"], p, "dpz"))
                same(np.float64(h["dE"]), dE[0], (hex(step), h["case"], p, "dE"))
                n_records += 1
        assert steps[f"s{i}_stats"][0] == 0           # no collision touched a velocity
    with capsys.disabled():
        print(f"\n[wall law] device velocities vs 40 digits, {n_hits} hits ({n_diffuse} diffuse, {n_specular} specular, {n_chained} specular "
              f"second hits): largest component error {worst:.3g} s (tolerance {VEL_RTOL:.3g} s)")
    assert n_hits > 1300 * len(STEPS) and n_specular > 50 * len(STEPS) and n_records > 1250 * len(STEPS)


def test_the_chosen_draws_are_among_the_hits(steps):
    """Every entry of the table is a good hit of its case at its step word, on the side of alpha it claims."""
    for kind, step, particle, case in H.TABLE:
        i = STEPS.index(step)
        mine = [h for h in hits_of(steps, i) if h["p"] == particle and h["case"] == case and h["ok"]]
        assert len(mine) == 1, (kind, hex(step), particle, case)
        if kind != "high_step":
            assert (mine[0]["Es"] != 0.0) == (not kind.endswith("_above")), (kind, hex(step), particle, case)


def test_counters_and_paths_are_the_reference_laws(steps, default):
    """What does not depend on the law: the hits themselves (particles, normals, contacts, ok), the counters and the emitted
    paths equal the reference law's on the same state — but for the second hits of the eight twice-hit particles."""
    s = DH.state()[0]
    corners = np.array(s.cases["draw_corner_4_8"])
    dt = np.dtype([("step", "<i4"), ("phase", "<i4"), ("cell", "<i8"), ("i", "<i4"), ("j", "<i4"), ("which", "<i4"), ("reserved", "<i4"),
                   ("total", "<f8"), ("px", "<f8"), ("py", "<f8"), ("pz", "<f8")])
    for i, step in enumerate(STEPS):
        for D in (steps, default):          # n_wall counts the records
            assert dict(zip(STAT_KEYS, D[f"s{i}_stats"].tolist()))["n_wall"] == sum(len(D[f"s{i}_draw_{case}_0"]) for case in CASES)
        for case in CASES:
            ka, kb = (~np.isin(D[f"s{i}_draw_{case}_0"], corners) if case >= 8 else slice(None) for D in (steps, default))
            for kind, k in (("draw", 0), ("draw", 1), ("draw", 2), ("con", 1), ("res", 3)):          # idx, normals, contact z, contacts, ok
                key = f"s{i}_{kind}_{case}_{k}"
                same(steps[key][ka], default[key][kb], (hex(step), case, kind, k))
        assert steps[f"s{i}_stats"][0] == default[f"s{i}_stats"][0] == 0, hex(step)          # n_pp
        pa, pb = (np.frombuffer(D[f"s{i}_paths"].tobytes(), dtype=dt) for D in (steps, default))
        pa, pb = pa[~np.isin(pa["i"], corners)], pb[~np.isin(pb["i"], corners)]
        assert len(pa) > 500 and pa.tobytes() == pb.tobytes(), (hex(step), len(pa), len(pb))


# ---- 2. alpha = 0 and alpha = 1 ----------------------------------------------------------------------------------------------------
def test_alpha_0_is_specular_bit_for_bit_and_alpha_1_is_diffuse():
    s, g, m = law_consts()
    v0 = np.stack([s.vx, s.vy, s.vz], axis=1)
    a0, a1 = JOBS["alpha0"](), JOBS["alpha1"]()
    for i, step in enumerate(FEW):
        vel = np.stack([a0[f"s{i}_state_{k}"] for k in ("vx", "vy", "vz")], axis=1)
        cur, n = v0.copy(), 0
        for h in hits_of(a0, i):
            if not h["ok"]:
                continue
            assert h["Es"] == 0.0, (hex(step), h["p"])
            cur[h["p"]] = W.specular(cur[h["p"]], h["normal"])          # (no libm call: the mirror's bits are the device's)
            n += 1
        same(vel, cur, (hex(step), "alpha 0"))
        assert n > 1300
        h1 = [h for h in hits_of(a1, i) if h["ok"]]
        assert len(h1) > 1300 and all(h["Es"] != 0.0 for h in h1), hex(step)
        w = np.stack([a1[f"s{i}_state_{k}"] for k in ("vx", "vy", "vz")], axis=1)
        last = [h for h in h1 if h["nth"] == h["of"]]
        assert all(float(w[h["p"]] @ h["normal"]) >= 0.0 for h in last)          # every one leaves the wall


# ---- 3. the other forms -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["AMC_TEMP_UNFUSED", "run", "AMC_TEMP_RUN_UNFUSED"])
def test_other_forms_draw_the_same(steps, tmp_path, form):
    if form == "run":
        other = JOBS["run"]()
    else:
        other = child("steps" if form == "AMC_TEMP_UNFUSED" else "run", {form: "1"}, tmp_path)
    assert_same(other, steps, form)


# ---- 4. back to the default --------------------------------------------------------------------------------------------------------
def test_taking_the_law_back_restores_the_default_bit_for_bit(default):
    assert_same(JOBS["back"](), default, "back")


# ---- 5. a longer run: shards, checkpoint, surfaces ---------------------------------------------------------------------------------
RUN_STEPS, N_RUN, DT_SCALE = 24, 6_000, 50.0
N_UNEVEN = N_RUN + 1         # over three ranks: 2,001 + 2,000 + 2,000


def _params(n=N_RUN):
    p, c = PR.pore_params(n=n, energised=True, sigma=3.6e-19 * 64.0)
    p.detect_mode = 1
    return p, c


def _sim(ic_seed=13, n=N_RUN):
    """the dense energised pore of tests/test_gpu_samplers_together.py: N = 6,000, fifty times the step, 64 times the cross section"""
    from argon_monte_carlo_amd.sim import TemperatureSimulation
    p, c = _params(n)
    sim = TemperatureSimulation(params=p, consts=c, np_rng=np.random.RandomState(3), py_rng=random.Random(3), device_rng_seed=7)
    sim.dt = DT_SCALE * c["dt"]
    sim.set_state(*IC.pore_ic(p, c, ic_seed))
    sim.enable_surface()
    return sim


def _series(sim):
    return np.array([[float(v) for v in sim.momentum_z_change_per_step], [float(v) for v in sim.energy_transfer_cold_per_step],
                     [float(v) for v in sim.energy_transfer_hot_per_step]]).T.copy(), np.array(sim._zero_flags, dtype=bool)


def _outcome(sim):
    series, zero = _series(sim)
    tot, nf, ns = sim.engine.surface_read()
    out = {f"state_{k}": v for k, v in sim.engine.download().items()}
    out.update(series=series, zero=zero, surf_totals=tot, surf_failed=nf, surf_steps=np.array([ns]))
    return out


def _long_run(n):
    sim = _sim(n=n)
    sim.set_wall_law("maxwell")
    assert sim.wall_law() == ("maxwell", 0.95, 0.8)              # (alpha defaults to the parameters')
    st = sim.run(RUN_STEPS)
    out = _outcome(sim)
    sim.close()
    count = np.array(SREF.from_words(out["surf_totals"]))[:, :, 0].sum(axis=1)
    assert st["n_wall"] > 0 and st["n_pp"] > 0 and int(count.sum()) > 0, (st, count)          # hits occur
    assert out["series"][:, 0].any()
    return out


@pytest.fixture(scope="module")
def long_run():
    return _long_run(N_RUN)


def test_long_run_differs_from_the_reference_law(long_run):
    sim = _sim()
    sim.run(RUN_STEPS)
    out = _outcome(sim)
    sim.close()
    assert not np.array_equal(out["state_vx"], long_run["state_vx"]) and not np.array_equal(out["series"], long_run["series"])


def test_single_steps_and_the_surface_reference_on_the_devices_records(long_run, capsys):
    """24 single steps under the law: the run's series, state and surface totals; and the totals are tests/surface_ref.py fed
    every step's hit records as the device returns them."""
    from tests.test_gpu_surface import step_records
    sim = _sim()
    sim.set_wall_law("maxwell", 0.95, 0.8)
    g = sim.engine.surface_grid
    nbins, lo, hi = int(g.nbins), list(g.lo), list(g.hi)
    tot, failed = SREF.empty(nbins)
    n_diffuse = n_specular = 0
    for _ in range(RUN_STEPS):
        sim.timestep(collect_paths=False)
        SREF.accumulate(tot, failed, nbins, lo, hi, step_records(sim.engine))
        for case in CASES:
            Es, ok = sim.engine.device_draws(case)[4], sim.engine.device_results(case)[3]
            n_diffuse, n_specular = n_diffuse + int((Es[ok] != 0).sum()), n_specular + int((Es[ok] == 0).sum())
    out = _outcome(sim)
    sim.close()
    assert_same(out, long_run, "single steps")
    assert np.array_equal(long_run["surf_totals"], SREF.to_words(tot)) and long_run["surf_failed"].tolist() == failed
    with capsys.disabled():
        print(f"\n[wall law] long run: {n_diffuse} diffuse and {n_specular} specular hits in {RUN_STEPS} steps")
    count = np.array(SREF.from_words(long_run["surf_totals"]))[:, :, 0].sum()
    assert n_diffuse > 0 and n_diffuse + n_specular == int(count), (n_diffuse, n_specular, count)


def test_checkpoint_carries_the_law(long_run, tmp_path):
    a = _sim()
    a.set_wall_law("maxwell")
    a.run(11)
    ck = str(tmp_path / "law.npz")
    a.save_checkpoint(ck)
    a.close()
    assert np.load(ck)["wall_law"].tolist() == [1.0, 0.95, 0.8]
    b = _sim(ic_seed=99)                    # another state, the reference law: the checkpoint brings its own
    assert b.wall_law()[0] == "reference"
    b.load_checkpoint(ck)
    assert b.wall_law() == ("maxwell", 0.95, 0.8)
    b.run(13)
    assert_same(_outcome(b), long_run, "checkpoint")
    # a file without the key loads with the reference law
    plain = str(tmp_path / "plain.npz")
    b.set_wall_law(None)
    b.save_checkpoint(plain)
    assert "wall_law" not in np.load(plain).files
    b.set_wall_law("maxwell", 0.5, 0.5)
    b.load_checkpoint(plain)
    assert b.wall_law()[0] == "reference"
    b.close()


@pytest.mark.parametrize("n", [N_RUN, N_UNEVEN])
def test_three_ranks_equal_the_single_context(long_run, n):
    """Three ranks on one GPU (LocalRanks); every rank's driver sets the same law on its own context.  A rank's range is the
    driver's shard of the world size and no other (amc_mg_sweep checks it), so the ranges of N = 6,000 are three times 2,000:
    the uneven ranges are those of the same pore with one atom more, 2,001 + 2,000 + 2,000, against a run of its own."""
    from argon_monte_carlo_amd.dist import shard_range
    RANGES = [shard_range(n, r, 3) for r in range(3)]
    assert [hi - lo for lo, hi in RANGES] == ([2_000] * 3 if n == N_RUN else [2_001, 2_000, 2_000])
    long_run = long_run if n == N_RUN else _long_run(n)
    from argon_monte_carlo_amd.dist import LocalRanks, ShardedTemperatureSimulation
    from argon_monte_carlo_amd.energised import SurfaceEnergies, device_rng_config
    from argon_monte_carlo_amd import surface as SU
    from argon_monte_carlo_amd.engine import ShardEnergisedEngine
    p, c = _params(n)
    p.reserved0 |= 1
    en = SurfaceEnergies(c)
    p.E_cold, p.E_hot = en.cold, en.hot
    init = IC.pore_ic(p, c, 13)
    cfg, dt = device_rng_config(c, 7), DT_SCALE * c["dt"]
    stream = torch.cuda.current_stream().cuda_stream
    engs = [ShardEnergisedEngine(p, lo, hi) for lo, hi in RANGES]
    try:
        for r, e in enumerate(engs):
            e.set_stream(stream)
            e.upload(*init)
            e.surface_config(SU.default_grid(p))
            d = ShardedTemperatureSimulation(p, r, 3, engine=e, comm=object(), device_rng_seed=7, consts=c)
            d.set_wall_law("maxwell")
            assert e.wall_law_get() == (1, 0.95, 0.8)
        ranks = LocalRanks(engs)
        for e in engs:
            e.shard_run_begin(RUN_STEPS)
        for k in range(RUN_STEPS):
            ranks.step_device(dt, cfg, k)
        ends = [e.shard_run_end(RUN_STEPS) for e in engs]
        for r, (st, sums, had) in enumerate(ends):
            same(sums, long_run["series"], ("series of rank", r))
            assert np.array_equal(~had, long_run["zero"]), r
        for (lo, hi), e in zip(RANGES, engs):
            st = e.download()
            for k in SF + ["flag"]:
                same(st[k][lo:hi], long_run[f"state_{k}"][lo:hi], ("state", k, lo))
        reads = [e.surface_read() for e in engs]
        ints = [SREF.from_words(t) for t, _, _ in reads]
        tot = [[[sum(v[s][b][q] for v in ints) for q in range(3)] for b in range(reads[0][0].shape[1])] for s in range(7)]
        assert np.array_equal(SREF.to_words(tot), long_run["surf_totals"])
        assert sum(nf for _, nf, _ in reads).tolist() == long_run["surf_failed"].tolist() and all(ns == RUN_STEPS for _, _, ns in reads)
        assert sum(1 for t, _, _ in reads if t.any()) >= 2
    finally:
        for e in engs:
            e.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from argon_monte_carlo_amd._lib import ArgonMCError
    from argon_monte_carlo_amd.engine import Engine
    from argon_monte_carlo_amd.sim import TemperatureSimulation
    p, c = _params()
    host = TemperatureSimulation(params=p, consts=c, np_rng=np.random.RandomState(3), py_rng=random.Random(3))
    with pytest.raises(ValueError):
        host.set_wall_law("maxwell")                       # no device_rng_seed: the host hand-over is the reference's
    host.close()
    sim = _sim()
    sim.set_wall_law("maxwell", 0.25, 0.75)
    before = sim.engine.wall_law_get()
    assert before == (1, 0.25, 0.75)
    for bad in (dict(alpha_coated=-0.1), dict(alpha_coated=1.5), dict(alpha_coated=float("nan")), dict(alpha_gap=-0.1),
                dict(alpha_gap=1.5), dict(alpha_gap=float("nan"))):
        with pytest.raises(ArgonMCError) as e:
            sim.set_wall_law("maxwell", **bad)
        assert e.value.code == -1 and sim.engine.wall_law_get() == before, bad
    with pytest.raises(ArgonMCError) as e:
        sim.engine.wall_law(2, 0.5, 0.5)
    assert e.value.code == -1 and sim.engine.wall_law_get() == before
    with pytest.raises(ValueError):
        sim.set_wall_law("cercignani")
    from argon_monte_carlo_amd._abi import AmcWallLaw
    import ctypes as C
    for field, value in (("struct_size", 48), ("reserved", None)):
        law = AmcWallLaw()
        law.struct_size, law.kind, law.alpha_coated, law.alpha_gap = C.sizeof(AmcWallLaw), 1, 0.5, 0.5
        if field == "reserved":
            law.reserved[2] = 1.0
        else:
            law.struct_size = value
        assert sim.engine.lib.amc_temp_wall_law(sim.engine._ctx, C.byref(law)) == -1 and sim.engine.wall_law_get() == before, field
    sim.engine.reset_outputs()
    assert sim.engine.wall_law_get() == before             # amc_reset_outputs leaves the law alone
    sim.close()
    pp, _ = PR.pore_params(n=100)
    plain = Engine(pp)                                     # a specular pore: no law
    law = AmcWallLaw()
    law.struct_size, law.kind = C.sizeof(AmcWallLaw), 1
    assert plain.lib.amc_temp_wall_law(plain._ctx, C.byref(law)) == -6 and plain.lib.amc_temp_wall_law_get(plain._ctx, C.byref(law)) == -6
    plain.close()


if __name__ == "__main__":
    np.savez(sys.argv[2], **JOBS[sys.argv[1]]())
