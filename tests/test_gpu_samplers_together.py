"""GPU (-m gpu): every sampler at once.  Fields, correlations, fluxes, velocity distributions, transits and the pair distribution
run on the mixed cadences of tests/together_states.py — inside one run() some steps are sampled by several of them behind one
streaming pass and some by nobody, so the pore's post-sweep bounds pass is deferred and not deferred in every order — beside the
free paths and, in the energised pore, the surfaces.  The reference is a twin context without a sampler, stepped one timestep()
at a time and downloaded after every step: each sampler's exact mirror (tests/*_ref.py) is fed the downloads of its own due
steps.  Every comparison is integer or byte equality.  Then the ways to drive the same steps — split runs, single steps, a
checkpoint in the middle, three ranks on one GPU, samplers switched off and on between runs — and, with the context's count of
owned objects (amc_owned_count), that a sampler gives back exactly what it allocated."""
import random

import numpy as np
import pytest
import torch                # (first: the library then shares torch's HIP runtime — the three ranks exchange through torch)

from argon_monte_carlo_amd import correlations as CO
from argon_monte_carlo_amd import distributions as VD
from argon_monte_carlo_amd import fields as FL
from argon_monte_carlo_amd import fluxes as FX
from argon_monte_carlo_amd import free_paths as FP
from argon_monte_carlo_amd import ic as IC
from argon_monte_carlo_amd import pairs as PA
from argon_monte_carlo_amd import params as PR
from argon_monte_carlo_amd import surface as SU
from argon_monte_carlo_amd import transits as TR
from argon_monte_carlo_amd._lib import ArgonMCError
from argon_monte_carlo_amd.totals import ints_to_words, words_to_ints
from tests import corr_ref as CREF
from tests import fields_ref as FREF
from tests import flux_ref as XREF
from tests import mfp_ref as MREF
from tests import pair_ref as PREF
from tests import together_states as TS
from tests import transit_ref as TREF
from tests import vdf_ref as VREF
from tests.sampler_states import ODD_N
from tests.test_gpu_pair import _dense_cube, _dense_pore

pytestmark = pytest.mark.gpu

KEYS = ("x", "y", "z", "vx", "vy", "vz", "d", "dx", "dy", "dz", "flag")
COUNTERS = ("n_pp", "n_wall", "n_oob_walls", "n_oob_pp", "n_paths", "n_fp_errors")
STEPS = TS.STEPS
NAMES = tuple(TS.MIX)                                   # the six samplers on a cadence, in the hook's order but for the free paths
MODS = {"fields": FL, "correlations": CO, "fluxes": FX, "distributions": VD, "transits": TR, "pairs": PA, "free_paths": FP, "surfaces": SU}
PREFIX = {"fields": "fields", "correlations": "corr", "fluxes": "flux", "distributions": "vdf", "transits": "transit", "pairs": "pair",
          "free_paths": "mfp", "surfaces": "surface"}
GRID_ATTR = {"fields": "field_grid", "correlations": "corr_grid", "fluxes": "flux_grid", "distributions": "vdf_grid",
             "transits": "transit_grid", "pairs": "pair_grid", "free_paths": "mfp_grid", "surfaces": "surface_grid"}
GRID_KEYS = ("fields_grid", "corr_grid", "flux_grid", "mfp_grid", "vdf_grid", "transit_grid", "pair_grid")
BLOCKS3 = {k: "3" for k in ("AMC_FIELDS_BLOCKS", "AMC_CORR_BLOCKS", "AMC_FLUX_BLOCKS", "AMC_VDF_BLOCKS", "AMC_TRANSIT_BLOCKS", "AMC_PAIR_BLOCKS")}
EVERY_STEP = {name: (1, 0) for name in NAMES}
N_SAMPLES = {"correlations": 1, "free_paths": 2}         # where a read's counters have the samples (steps) taken; the others first
MANUAL = {name: (0, 0) for name in NAMES}
# The pores' own time step moves an atom 0.07 nm: in 24 such steps no atom of these few thousand meets a wall, and after the first
# step (the initial condition's overlapping pairs) none meets another.  With fifty times the step — 3.5 nm, about a collision range —
# every step has collisions and wall hits, and the post-sweep bounds pass moves particles on sampled steps inside the run.
PORE_DT_SCALE = 50.0


# ---- contexts, grids, reads -------------------------------------------------------------------------------------------------------
def _lead(geom):
    """"pore+7": the context has taken seven steps before the initial state is uploaded (again) and the samplers are configured"""
    return int(geom.split("+")[1]) if "+" in geom else 0


def _new(geom, seed=None):
    """The dense cube (N = 3,000, sixteen times the cross section) or the dense pore (N = 8,000, 64 times) of tests/test_gpu_pair.py.
    "pore+7": the step counter stands at 7 when the run begins, so the run's first step — the one in which the initial
    condition's overlapping pairs collide, and the only one whose post-sweep bounds pass moves particles (two of them) — is step 8
    of the mix: sampled by three samplers at once, two of which count who is outside the domain, and followed by a sampled step
    inside the run."""
    from argon_monte_carlo_amd.sim import Simulation
    if geom == "cube":
        return _dense_cube() if seed is None else _dense_cube(seed=seed)
    p, c, init = _dense_pore()
    sim = Simulation("pore", params=p, consts=c)
    sim.dt = PORE_DT_SCALE * c["dt"]
    sim.set_state(*(init if seed is None else IC.pore_ic(p, c, seed)))
    for _ in range(_lead(geom)):
        sim.timestep(collect_paths=False)
    if _lead(geom):
        sim.engine.drain_paths()
        sim.set_state(*init)
    return sim


def _temp_new(ic_seed=13):
    """the energised pore of tests/test_gpu_pair.py's _temp_sim — N = 6,000, directions and gap energies drawn on the device — with
    64 times the cross section and PORE_DT_SCALE times the time step: atoms collide, hit the energised walls and complete free paths"""
    from argon_monte_carlo_amd.sim import TemperatureSimulation
    p, c = PR.pore_params(n=6_000, energised=True, sigma=3.6e-19 * 64.0)
    sim = TemperatureSimulation(params=p, consts=c, np_rng=np.random.RandomState(3), py_rng=random.Random(3), device_rng_seed=7)
    sim.dt = PORE_DT_SCALE * c["dt"]
    sim.set_state(*IC.pore_ic(p, c, ic_seed))
    return sim


def _grids(geom, p, label="A"):
    """name -> grid without a cadence; "B": every grid of another size.  Small pair grids (r_max = 8 collision ranges, at most 16
    columns): the mirror is O(N^2) per sample."""
    b = label == "B"
    if geom == "cube":
        lo, hi = (0.0, 0.0, 0.0), (p.cube_x, p.cube_y, p.cube_z)
        kind = "cartesian"
        n = dict(fields=(2, 2, 5), correlations=(1, 3, 1), fluxes=(1, 1, 2), distributions=(1, 2, 1), pairs=(1, 1, 1), free_paths=(3, 1, 2)) if b else \
            dict(fields=(3, 2, 2), correlations=(2, 1, 1), fluxes=(2, 3, 1), distributions=(2, 1, 2), pairs=(2, 1, 2), free_paths=(2, 2, 1))
        zones = [(1, 0.25 * p.cube_y, 0.75 * p.cube_y), (2, 0.0, 0.5 * p.cube_z)] if b else TR.zones(TR.default_grid(p))
    else:
        lo, hi = (0.0, 0.0), (p.R_oa, p.H)
        kind = "axisymmetric"
        n = dict(fields=(3, 7), correlations=(2, 2), fluxes=(1, 3), distributions=(2, 2), pairs=(1, 2), free_paths=(1, 6)) if b else \
            dict(fields=(2, 5), correlations=(1, 3), fluxes=(2, 4), distributions=(1, 4), pairs=(1, 4), free_paths=(2, 4))
        zones = [(2, 0.25 * p.H, 0.5 * p.H)] if b else [(2, p.h_oa, p.h_oa + 2e-9), (2, 0.0, 0.25 * p.H), (0, -0.5 * p.R_oa, 0.5 * p.R_oa)]
    r_max = 8.0 * float(p.collision_range)
    out = {"fields": FL.make_grid(kind, n["fields"], lo, hi),
           "correlations": CO.make_grid(kind, n["correlations"], lo, hi, n_lags=3 if b else TS.N_LAGS),
           "fluxes": FX.make_grid(kind, n["fluxes"], lo, hi),
           "distributions": VD.make_grid(kind, n["distributions"], lo, hi, hist_bins=24 if b else 16),
           "transits": TR.make_grid(zones, every=0),
           "pairs": PA.make_grid(kind, n["pairs"], lo, hi, r_max, hist_bins=12 if b else 16),
           "free_paths": FP.make_grid(kind, n["free_paths"], lo, hi, hist_bins=12 if b else 8)}
    if geom == "temp":
        out["surfaces"] = SU.default_grid(p, 4 if b else 8)
    return out


def _config(engine, name, grid, cadence=(0, 0), keep=False):
    if name == "free_paths":
        engine.mfp_config(None if grid is None else FP.copy_grid(grid, keep_records=keep))
    elif name == "surfaces":
        engine.surface_config(grid)
    else:
        getattr(engine, PREFIX[name] + "_config")(None if grid is None else MODS[name].copy_grid(grid, every=cadence[0], step_offset=cadence[1]))


def _configure(engine, grids, mix=None, mfp=None, surfaces=False):
    """the six cadence samplers on ``mix``; mfp: None (off) or keep_records; the surfaces"""
    mix = TS.MIX if mix is None else mix
    for name in NAMES:
        _config(engine, name, grids[name], mix[name])
    if mfp is not None:
        _config(engine, "free_paths", grids["free_paths"], keep=mfp)
    if surfaces:
        _config(engine, "surfaces", grids["surfaces"])


def _inside_entries(state, entry):
    """the entry indices of the particles inside a zone (the others' are not specified), the rest zero"""
    out = np.array(entry, dtype=np.uint32)
    for k in range(out.shape[0]):
        out[k][((state >> np.uint32(4 * k)) & np.uint32(3)) != 2] = 0
    return out


def _read(e, name, per_particle=True):
    """a sampler's totals, counters and, per_particle, what it remembers of every particle: a dict of arrays and tuples"""
    if name in ("fields", "fluxes", "distributions"):
        tot, ns, no = getattr(e, PREFIX[name] + "_read")()
        return dict(totals=tot, counters=(ns, no))
    if name == "correlations":
        tot, c = e.corr_read()
        out = dict(totals=tot, counters=tuple(c))
        if per_particle:
            out["origin"] = np.stack(e.corr_origin())
        return out
    if name == "transits":
        tot, ns = e.transit_read()
        out = dict(totals=tot, counters=(ns,))
        if per_particle:
            state, entry = e.transit_state()
            out.update(state=state, entry=_inside_entries(state, entry))
        return out
    if name == "pairs":
        tot, ns, no, nu = e.pair_read()
        return dict(totals=tot, counters=(ns, no, nu))
    if name == "free_paths":
        tot, hist, c = e.mfp_read()
        return dict(totals=tot, hist=hist, counters=tuple(c))
    tot, nf, ns = e.surface_read()
    return dict(totals=tot, failed=nf, counters=(ns,))


def _same(got, want, what):
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for k, w in want.items():
        g = got[k]
        if isinstance(w, tuple):
            assert tuple(int(v) for v in g) == tuple(int(v) for v in w), (what, k, g, w)
        else:
            assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
            assert g.tobytes() == w.tobytes(), (what, k, np.argwhere(np.asarray(g != w))[:5])


# ---- the twin and the mirrors ---------------------------------------------------------------------------------------------------------
_TRACE, _MIRROR = {}, {}


def _trace(geom):
    """The twin without a sampler: 24 timestep() calls, after each the drained path records and the downloaded state; at the end
    the summed statistics and the device histograms.  Once per geometry, never changed."""
    if geom not in _TRACE:
        sim = _new(geom)
        states, records, per_step = [], [], []
        for _ in range(STEPS):
            per_step.append(sim.timestep(collect_paths=False))
            records.append(sim.engine.drain_paths(sort=False))
            states.append(sim.engine.download())
        total = _sum_stats(per_step)
        counts, npaths = sim.engine.histograms()
        _TRACE[geom] = dict(states=states, records=records, stats=total, per_step=per_step, hist=counts, npaths=npaths)
        sim.close()
        assert sum(1 for st in per_step if st["n_pp"] >= 1) >= STEPS // 2 and total["n_paths"] >= 1, [st["n_pp"] for st in per_step]
    return _TRACE[geom]


def _mirror(geom, name, grid, steps, label="A"):
    """what _read returns, from the sampler's mirror fed the twin's states of ``steps`` (1-based, in order); cached"""
    key = (geom, name, label, tuple(steps))
    if key in _MIRROR:
        return _MIRROR[key]
    tr = _temp_trace() if geom == "temp" else _trace(geom)
    states = tr["states"]
    if name == "fields":
        sums, outside = np.zeros((FL.grid_bins(grid), 7), dtype=object), 0
        for s in steps:
            a, o = FREF.sample_state(grid, states[s - 1])
            sums, outside = sums + a, outside + o
        out = dict(totals=FL.ints_to_words(sums), counters=(len(steps), outside))
    elif name == "correlations":
        w = CREF.Window(grid)
        for s in steps:
            w.add(CREF.state6(states[s - 1]))
        out = dict(totals=w.words(), counters=w.counters(), origin=np.stack(w.origin))
    elif name == "fluxes":
        t = XREF.Totals(grid)
        for s in steps:
            t.add_state(states[s - 1])
        out = dict(totals=t.words(), counters=(t.n_samples, t.n_outside))
    elif name == "distributions":
        t = VREF.Totals(grid)
        for s in steps:
            t.add_state(states[s - 1])
        VREF.check_invariants(grid, t.sums)
        out = dict(totals=t.sums, counters=(t.n_samples, t.n_outside))
    elif name == "transits":
        m = TREF.Mirror(TR.zones(grid), len(states[0]["x"]))
        for s in steps:
            m.sample(states[s - 1]["x"], states[s - 1]["y"], states[s - 1]["z"])
        assert m.bad is None and not m.over
        out = dict(totals=m.words(), counters=(m.n_samples,), state=m.state, entry=_inside_entries(m.state, m.entry))
    elif name == "pairs":
        t = PREF.Totals(grid)
        for s in steps:
            t.add_state(states[s - 1])
        out = dict(totals=t.sums, counters=(t.n_samples, t.n_outside, t.n_unfiled))
    else:
        assert name == "free_paths"
        t = MREF.Totals(grid)
        for s in steps:
            t.add_step(tr["records"][s - 1], states[s - 1])
        t.check()
        out = dict(totals=t.words(), hist=t.hist, counters=t.counters())
    _MIRROR[key] = out
    return out


def _check_samplers(engine, geom, grids, mfp=False, first=1, names=NAMES):
    """every cadence sampler (and the free paths) against its mirror over the steps first .. 24; nothing compares zeros"""
    lead = _lead(geom)
    for name in names:
        want = _mirror(geom, name, grids[name], [s - lead for s in TS.due_steps(name, first + lead, STEPS + lead)])
        assert want["totals"].any() and want["counters"][0] >= 2, name
        _same(_read(engine, name), want, name)
    if mfp:
        want = _mirror(geom, "free_paths", grids["free_paths"], list(range(first, STEPS + 1)))
        assert want["counters"][0] > 0 and want["totals"].any() and want["hist"].any()
        _same(_read(engine, "free_paths"), want, "free_paths")


def _check_twin(sim, tr, stats=None):
    """the final state, the summed step statistics, the device histograms and the number of paths are the twin's, byte for byte"""
    st = sim.engine.download()
    for k in KEYS:
        assert st[k].tobytes() == tr["states"][-1][k].tobytes(), k
    if stats is not None:
        assert {k: stats[k] for k in COUNTERS} == tr["stats"], (stats, tr["stats"])
    counts, npaths = sim.engine.histograms()
    base = getattr(sim, "_hist_base", None)     # (a resumed run: the paths completed before the checkpoint)
    if base is not None:
        counts, npaths = counts + base, npaths + int(base[0].sum())
    assert npaths == tr["npaths"] and counts.tobytes() == tr["hist"].tobytes()


def _sum_stats(stats):
    return {k: sum(s[k] for s in stats) for k in COUNTERS}


# ---- 1. mixed cadences in one run -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom,env", [("cube", {}), ("pore", {}), ("pore+7", {}), ("pore+7", {"AMC_LIST_KEEP": "4"}), ("cube", {"AMC_OVERLAP": "1"}),
                                      ("pore+7", {"AMC_OVERLAP": "1"}), ("cube", BLOCKS3), ("pore+7", BLOCKS3)],
                         ids=["cube", "pore", "pore+7", "pore+7-list_keep4", "cube-overlap", "pore+7-overlap", "cube-blocks3", "pore+7-blocks3"])
def test_mixed_cadences_in_one_run(geom, env, monkeypatch):
    """Free paths off: in the pore the bounds pass of a step nobody samples is left to the next step's pass, in every order of
    sampled and idle steps.  A deferral in front of a due step would have a sampler read the state from before the bounds pass —
    which shows only where that pass moves a particle: "pore+7" (see _new)."""
    tr = _trace(geom)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if _lead(geom):                         # a sampled step inside the run whose bounds pass, after the sweep, moved a particle: deferred, the sample would miss it
        moved = [s for s in range(1, STEPS) if TS.due_names(s + _lead(geom)) and tr["per_step"][s - 1]["n_oob_pp"] >= 1]
        print("sampled steps whose post-sweep bounds pass moved a particle:", moved)
        assert moved, [st["n_oob_pp"] for st in tr["per_step"]]
    sim = _new(geom)
    grids = _grids(geom, sim.params)
    _configure(sim.engine, grids)
    stats = sim.run(STEPS)
    _check_samplers(sim.engine, geom, grids)
    _check_twin(sim, tr, stats)
    if "AMC_OVERLAP" in env:                # the opt-in is on, and a run with samplers on a cadence takes the plain loop all the same
        ov = sim.engine.overlap_stats()
        assert ov["mode"] == 1 and ov["steps"] == 0, ov
    if "AMC_LIST_KEEP" in env:
        assert sim.engine.lists_stats()["keep_K"] == 4
    sim.close()


# ---- 2. ... beside the free paths: every step is due ----------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", ["cube", "pore"])
@pytest.mark.parametrize("keep", [False, True], ids=["consume", "keep_records"])
def test_mixed_cadences_beside_the_free_paths(geom, keep):
    tr = _trace(geom)
    sim = _new(geom)
    grids = _grids(geom, sim.params)
    _configure(sim.engine, grids, mfp=keep)
    stats = sim.run(STEPS)
    _check_samplers(sim.engine, geom, grids, mfp=True)
    _check_twin(sim, tr, stats)
    if keep:                                # the records are still there, and they are the twin's
        got = sim.engine.drain_paths(sort=True)
        want = np.concatenate(tr["records"])
        want = want[np.lexsort((want["which"], want["j"], want["i"], want["cell"], want["phase"], want["step"]))]
        assert len(got) == len(want) > 0 and got.tobytes() == want.tobytes()
    else:
        assert sim.engine.paths_pending() == 0 and len(sim.engine.drain_paths()) == 0
    sim.close()


# ---- 3. split runs and single steps -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", ["cube", "pore"])
@pytest.mark.parametrize("parts", [(7, 8, 9), (1,) * STEPS], ids=["run7_8_9", "timesteps"])
def test_split_runs_and_single_steps_give_the_totals_of_one_run(geom, parts):
    """(the totals of run(24) are the mirrors': tests 1 and 2)"""
    tr = _trace(geom)
    sim = _new(geom)
    grids = _grids(geom, sim.params)
    _configure(sim.engine, grids, mfp=False)
    stats = [sim.timestep(collect_paths=False) if k == 1 else sim.run(k) for k in parts]
    assert sum(parts) == STEPS
    _check_samplers(sim.engine, geom, grids, mfp=True)
    _check_twin(sim, tr, _sum_stats(stats))
    sim.close()


# ---- 4. a checkpoint with everything on -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", ["cube", "pore"])
def test_checkpoint_with_everything_on_resumes_to_the_uninterrupted_totals(geom, tmp_path):
    tr = _trace(geom)
    a = _new(geom)
    grids = _grids(geom, a.params)
    _configure(a.engine, grids, mfp=False)
    a.run(11)
    ck = str(tmp_path / "all.npz")
    a.save_checkpoint(ck)
    a.close()
    files = list(np.load(ck).files)
    assert all(files.count(k) == 1 for k in GRID_KEYS), files
    b = _new(geom, seed=99)                 # another state: the checkpoint brings its own
    b.load_checkpoint(ck)
    for name in NAMES + ("free_paths",):
        assert getattr(b.engine, GRID_ATTR[name]) is not None, name
    b.run(13)
    _check_samplers(b.engine, geom, grids, mfp=True)
    st = b.engine.download()
    for k in KEYS:
        assert st[k].tobytes() == tr["states"][-1][k].tobytes(), k
    b.close()
    # a checkpoint without any sampler turns every one off
    c = _new(geom)
    c.run(1)
    plain = str(tmp_path / "plain.npz")
    c.save_checkpoint(plain)
    assert not set(GRID_KEYS) & set(np.load(plain).files)
    _configure(c.engine, grids, mfp=True)
    c.load_checkpoint(plain)
    for name in NAMES + ("free_paths",):
        assert getattr(c.engine, GRID_ATTR[name]) is None, name
        with pytest.raises(ArgonMCError) as e:
            _read(c.engine, name)
        assert e.value.code == -6, name
    c.close()


# ---- 4b. the checkpoint format: exactly these keys, dtypes and shapes ---------------------------------------------------------------------
# what a checkpoint holds without any sampler: the cube / pores, and what the energised pore adds
PLAIN_KEYS = {"kind", "n", "collision_range", "hist_counts", "completed_paths", "completed_x_paths", "completed_y_paths", "completed_z_paths",
              "total_cols", "steps_done", "device_step"} | {"state_" + k for k in KEYS}
TEMP_KEYS = {"momentum", "energy_cold", "energy_hot", "zero_flags", "total_errs", "np_rng_keys", "np_rng_rest", "np_rng_gauss", "py_rng_state",
             "py_rng_version"}
I8, U4, F8 = "int64", "uint32", "float64"


def _sampler_keys(n, bins):
    """key -> (dtype, shape) for the grids "A" of _grids: bins = (fields, correlation groups, fluxes, free paths) — the rest is the
    same in the cube and the energised pore: n_lags 2, 8 free-path columns, 4 regions of 16 columns for the distributions and the
    pairs, 3 zones"""
    fl, co, fx, fp = bins
    return {"fields_grid": (F8, (12,)), "fields_totals": (I8, (fl, 7, 2)), "fields_n_samples": (I8, ()), "fields_n_outside": (I8, ()),
            "flux_grid": (F8, (12,)), "flux_totals": (I8, (fx, 2, 7, 2)), "flux_n_samples": (I8, ()), "flux_n_outside": (I8, ()),
            "corr_grid": (F8, (13,)), "corr_totals": (I8, (co, 3, 7, 2)), "corr_counters": (I8, (4,)), "corr_origin": (F8, (6, n)),
            "mfp_grid": (F8, (13,)), "mfp_totals": (I8, (fp, 2, 7, 2)), "mfp_hist": (I8, (fp, 2, 9)), "mfp_counters": (I8, (3,)),
            "vdf_grid": (F8, (14,)), "vdf_totals": (I8, (4, 72)), "vdf_counters": (I8, (2,)),
            "transit_grid": (F8, (27,)), "transit_totals": (I8, (3, 263, 2)), "transit_counters": (I8, (1,)), "transit_state": (U4, (n,)),
            "transit_entry": (U4, (3, n)),
            "pair_grid": (F8, (14,)), "pair_totals": (I8, (4, 33)), "pair_counters": (I8, (3,))}


SURFACE_KEYS = {"surface_grid": (F8, (15,)), "surface_totals": (I8, (7, 9, 3, 2)), "surface_n_failed": (I8, (7,)), "surface_n_steps": (I8, ())}


@pytest.mark.parametrize("geom", ["cube", "temp"])
def test_a_checkpoint_holds_exactly_the_frozen_keys(geom, tmp_path):
    """Two steps with every sampler on (the energised pore: the surfaces too), then the file's keys, dtypes and shapes; a simulation
    with no sampler on writes none of the samplers' keys."""
    temp = geom == "temp"
    sim = _temp_new() if temp else _new(geom)
    n = int(sim.params.n)
    want = _sampler_keys(n, (10, 3, 8, 8) if temp else (12, 2, 6, 4))
    if temp:
        want.update(SURFACE_KEYS)
    plain = PLAIN_KEYS | (TEMP_KEYS if temp else set())
    assert n == (6_000 if temp else 3_000) and len(want) == (31 if temp else 27) and not set(want) & plain
    off = str(tmp_path / "off.npz")
    sim.save_checkpoint(off)
    assert set(np.load(off).files) == plain
    _configure(sim.engine, _grids(geom, sim.params), mix=EVERY_STEP, mfp=False, surfaces=temp)
    sim.run(2)
    on = str(tmp_path / "on.npz")
    sim.save_checkpoint(on)
    z = np.load(on)
    assert set(z.files) == plain | set(want), (sorted(set(z.files) - plain - set(want)), sorted((plain | set(want)) - set(z.files)))
    for k, (dtype, shape) in want.items():
        assert z[k].dtype == np.dtype(dtype) and z[k].shape == shape, (k, z[k].dtype, z[k].shape)
    assert int(z["fields_n_samples"]) == int(z["flux_n_samples"]) == 2 and z["vdf_counters"][0] == z["transit_counters"][0] == z["pair_counters"][0] == 2
    assert z["corr_counters"][1] == 2 and z["mfp_counters"][2] == 2 and (not temp or int(z["surface_n_steps"]) == 2)
    sim.close()


# ---- 5. the energised pore, directions and gap energies drawn on the device ---------------------------------------------------------------
_TEMP = {}


def _temp_trace():
    """The energised twin: surfaces and free paths (keeping the records) on, the six others with every = 0; 24 timestep() calls,
    after each the manual samples of the samplers due, the download and the drained records."""
    if not _TEMP:
        sim = _temp_new()
        grids = _grids("temp", sim.params)
        _configure(sim.engine, grids, mix=MANUAL, mfp=True, surfaces=True)
        states, records, per_step = [], [], []
        for s in range(1, STEPS + 1):
            per_step.append(sim.timestep(collect_paths=False))
            for name in TS.due_names(s):
                getattr(sim.engine, PREFIX[name] + "_sample")()
            states.append(sim.engine.download())
            records.append(sim.engine.drain_paths(sort=False))
        total = _sum_stats(per_step)
        counts, npaths = sim.engine.histograms()
        _TEMP.update(states=states, records=records, stats=total, per_step=per_step, hist=counts, npaths=npaths, grids=grids,
                     reads={name: _read(sim.engine, name) for name in NAMES + ("free_paths", "surfaces")},
                     series=(list(sim.momentum_z_change_per_step), list(sim.energy_transfer_cold_per_step), list(sim.energy_transfer_hot_per_step)),
                     zero_flags=list(sim._zero_flags))
        sim.close()
        assert sum(1 for st in per_step if st["n_pp"] >= 1) >= STEPS // 2 and total["n_wall"] >= 1, [(st["n_pp"], st["n_wall"]) for st in per_step]
        assert _TEMP["reads"]["surfaces"]["totals"].any() and any(v != 0 for v in _TEMP["series"][0])
    return _TEMP


def _check_temp(sim, tr, mfp, stats=None):
    grids = tr["grids"]
    _check_samplers(sim.engine, "temp", grids, mfp=mfp)
    for name in NAMES + (("free_paths",) if mfp else ()) + ("surfaces",):      # ... and the twin's own manual samples
        _same(_read(sim.engine, name), tr["reads"][name], "twin " + name)
    got = (sim.momentum_z_change_per_step, sim.energy_transfer_cold_per_step, sim.energy_transfer_hot_per_step)
    for g, w in zip(got, tr["series"]):
        assert len(g) == STEPS and np.array(g, dtype=np.float64).tobytes() == np.array(w, dtype=np.float64).tobytes()
    assert [tuple(bool(v) for v in row) for row in sim._zero_flags] == [tuple(bool(v) for v in row) for row in tr["zero_flags"]]
    _check_twin(sim, tr, stats)


@pytest.mark.parametrize("unfused,mfp", [(False, True), (True, True), (False, False)], ids=["fused", "unfused", "fused-no_free_paths"])
def test_energised_run_with_everything_on(unfused, mfp, monkeypatch):
    """Without the free paths the fused pass leaves the recapture of an idle step to the next one, as the plain loop does."""
    tr = _temp_trace()
    if unfused:
        monkeypatch.setenv("AMC_TEMP_RUN_UNFUSED", "1")
    sim = _temp_new()
    _configure(sim.engine, tr["grids"], mfp=False if mfp else None, surfaces=True)
    stats = sim.run(STEPS)
    _check_temp(sim, tr, mfp, stats)
    sim.close()


def test_energised_checkpoint_at_step_11_resumes_to_the_same_totals(tmp_path):
    """The resumed device-RNG run counts its steps on from the checkpoint's (set_step): the cadences keep their offsets."""
    tr = _temp_trace()
    a = _temp_new()
    _configure(a.engine, tr["grids"], mfp=False, surfaces=True)
    a.run(11)
    ck = str(tmp_path / "temp.npz")
    a.save_checkpoint(ck)
    a.close()
    files = list(np.load(ck).files)
    assert all(files.count(k) == 1 for k in GRID_KEYS + ("surface_grid",)), files
    b = _temp_new(ic_seed=99)
    b.load_checkpoint(ck)
    b.run(13)
    _check_temp(b, tr, True)
    b.close()
    # a checkpoint without any sampler, loaded into a simulation that has all eight on, turns every one off
    c = _temp_new()
    c.run(1)
    plain = str(tmp_path / "plain.npz")
    c.save_checkpoint(plain)
    _configure(c.engine, tr["grids"], mfp=True, surfaces=True)
    c.load_checkpoint(plain)
    for name in NAMES + ("free_paths", "surfaces"):
        assert getattr(c.engine, GRID_ATTR[name]) is None, name
        with pytest.raises(ArgonMCError) as e:
            _read(c.engine, name)
        assert e.value.code == -6, name
    c.close()


# ---- 6. three ranks with uneven ranges on one GPU ---------------------------------------------------------------------------------------
def _sum_words(parts):
    return ints_to_words(sum(words_to_ints(p) for p in parts))


# which counters of a sampler add up over the ranks (the others are the same on every rank)
_SUMMED = {"fields": (1,), "fluxes": (1,), "distributions": (1,), "correlations": (2,), "transits": (), "pairs": (1,), "free_paths": (0, 1)}
_WORDS = ("fields", "fluxes", "correlations", "transits", "free_paths")       # 128-bit (low, high) totals; the others plain int64


def _sum_over_ranks(name, reads):
    out = dict(totals=_sum_words([r["totals"] for r in reads]) if name in _WORDS else sum(r["totals"] for r in reads))
    if name == "free_paths":
        out["hist"] = sum(r["hist"] for r in reads)
    cs = [r["counters"] for r in reads]
    for k in range(len(cs[0])):
        if k not in _SUMMED[name]:
            assert len({c[k] for c in cs}) == 1, (name, k, cs)
    out["counters"] = tuple(sum(c[k] for c in cs) if k in _SUMMED[name] else cs[0][k] for k in range(len(cs[0])))
    return out


@pytest.mark.parametrize("geom", ["cube", "pore"])
def test_three_ranks_sum_to_the_single_context(geom):
    """Cube (N = 3,001): all seven.  Pore (N = 8,000: fewer atoms complete no free path in 24 steps): all but the pair distribution,
    which an index-range shard of a pore refuses.  Then one step more, around which the sharded driver switches four samplers
    on and off: every rank's context owns what it owned before."""
    from argon_monte_carlo_amd.dist import LocalRanks, ShardedSimulation, shard_range
    from argon_monte_carlo_amd.engine import Engine, ShardEngine
    if geom == "cube":
        n = 3001
        p, c = PR.cube_params_for_n(n, sigma=3.6e-19 * 16.0)
        p.detect_mode = 1
        init = IC.cube_ic(p, c, 10)
    else:
        n = 8000
        p, c, init = _dense_pore(n)
    dt = c["dt"] * (1.0 if geom == "cube" else PORE_DT_SCALE)
    names = tuple(k for k in NAMES if geom == "cube" or k != "pairs") + ("free_paths",)
    grids = _grids(geom, p)

    def configure(e):
        for name in names:
            _config(e, name, grids[name], TS.MIX.get(name, (0, 0)))
    one = Engine(p)
    one.upload(*init)
    configure(one)
    assert one.run(dt, STEPS)["n_pp"] >= 1
    want = {name: _read(one, name, per_particle=False) for name in names}
    end = one.download()
    one.close()
    for name in names:
        assert want[name]["totals"].any() and want[name]["counters"][0] >= 2, name
    ranges = [shard_range(n, r, 3) for r in range(3)]
    assert [hi - lo for lo, hi in ranges] == ([1001, 1000, 1000] if geom == "cube" else [2667, 2667, 2666])
    stream = torch.cuda.current_stream().cuda_stream
    engs = [ShardEngine(p, lo, hi) for lo, hi in ranges]
    for e in engs:
        e.set_stream(stream)
        e.upload(*init)
        configure(e)
    job = LocalRanks(engs)
    for _ in range(STEPS):
        job.step(dt)
    for name in names:
        reads = [_read(e, name, per_particle=False) for e in engs]
        _same(_sum_over_ranks(name, reads), want[name], name)
        assert sum(1 for r in reads if r["totals"].any()) >= (1 if name == "free_paths" else 2), name     # more than one rank has added to them
    for (lo, hi), e in zip(ranges, engs):   # every rank ends with its own range of the single context's state
        st = e.download()
        for k in ("x", "y", "z", "vx", "vy", "vz"):
            assert st[k][lo:hi].tobytes() == end[k][lo:hi].tobytes(), k
    # the driver's disable_* (the engines are its; it needs no communicator for this)
    four = ("fields", "correlations", "fluxes", "distributions")
    drivers = [ShardedSimulation(p, r, 3, engine=e, comm=object()) for r, e in enumerate(engs)]

    def switch_off(d):
        d.disable_fields(), d.disable_correlations(), d.disable_fluxes(), d.disable_distributions()
        assert all(getattr(d.engine, GRID_ATTR[name]) is None for name in four)
        return d.engine.owned_count()
    base = [switch_off(d) for d in drivers]
    for d in drivers:
        d.enable_fields(grids["fields"], every=1), d.enable_correlations(grids["correlations"], every=1)
        d.enable_fluxes(grids["fluxes"], every=1), d.enable_distributions(grids["distributions"], every=1)
        assert all(getattr(d.engine, GRID_ATTR[name]) is not None for name in four)
    assert all(d.engine.owned_count() >= b + 4 for d, b in zip(drivers, base))
    job.step(dt)
    for d in drivers:
        assert all(_read(d.engine, name, per_particle=False)["counters"][N_SAMPLES.get(name, 0)] == 1 for name in four)
    assert [switch_off(d) for d in drivers] == base
    for e in engs:
        e.close()


# ---- 7. the life cycle in the middle of a run -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", ["cube", "pore"])
def test_samplers_switched_off_and_on_between_two_runs(geom):
    """After 11 steps the transits (per-particle memory) and the fluxes (none) are switched off and the fluxes on again on another
    grid: the others' totals are those of the uninterrupted run, the fluxes start from zero and their cadence — every 5, no
    offset — counts from the run's first step: samples after the steps 15 and 20."""
    tr = _trace(geom)
    sim = _new(geom)
    grids = _grids(geom, sim.params)
    _configure(sim.engine, grids, mfp=False)
    sim.run(11)
    before = _read(sim.engine, "fluxes")
    assert before["counters"][0] == len(TS.due_steps("fluxes", 1, 11)) == 2
    sim.disable_transits()
    sim.disable_fluxes()
    other = _grids(geom, sim.params, "B")["fluxes"]
    sim.enable_fluxes(other, every=5)
    got = _read(sim.engine, "fluxes")
    assert got["counters"] == (0, 0) and not got["totals"].any() and got["totals"].shape != before["totals"].shape
    sim.run(13)
    _check_samplers(sim.engine, geom, grids, mfp=True, names=("fields", "correlations", "distributions", "pairs"))
    want = _mirror(geom, "fluxes", other, [15, 20], label="B")
    assert want["totals"].any()
    _same(_read(sim.engine, "fluxes"), want, "fluxes again")
    assert sim.engine.transit_grid is None
    with pytest.raises(ArgonMCError) as e:
        sim.engine.transit_read()
    assert e.value.code == -6
    _check_twin(sim, tr)
    sim.close()


# ---- 8. what a sampler allocates it gives back: the context's count of owned objects ---------------------------------------------------
def _mutations(name, g):
    """the sampler's invalid grids (those of its own tests), as changed copies of the valid grid g"""
    import math
    if name == "surfaces":
        out = [("struct_size", g.struct_size - 8), ("nbins", 0), ("nbins", 257)]
        ranges = [(0, (1.0, 1.0)), (3, (2.0, 1.0)), (6, (math.nan, 1.0)), (2, (0.0, math.inf))]
    else:
        out = {"fields": [("n1", 2049), ("kind", 2), ("every", -1)],
               "correlations": [("n1", 257), ("kind", 2), ("every", -1)],
               "fluxes": [("n1", 1025)],
               "distributions": [("n1", 1537), ("hist_bins", 257), ("hist_bins", 0), ("v_max", 0.0), ("v_max", math.inf), ("v_max", 16385.0)],
               "transits": [("n_zones", 0), ("n_zones", 9), ("every", -1), ("step_offset", -1), ("struct_size", 192)],
               "pairs": [("n1", 6145), ("hist_bins", 257), ("hist_bins", 0), ("r_max", 0.0), ("r_max", -1.0), ("r_max", math.inf), ("r_max", math.nan)],
               "free_paths": [("hist_bins", 65), ("hist_bins", -1), ("keep_records", 2), ("hist_hi", 0.0), ("hist_hi", -1e-6), ("hist_hi", math.inf),
                              ("hist_hi", math.nan), ("reserved", 1), ("kind", 2), ("n1", 0)]}[name]
        ranges = []
    bad = []
    for field, value in out:
        b = type(g).from_buffer_copy(g)
        setattr(b, field, value)
        bad.append(((field, value), b))
    for s, (lo, hi) in ranges:
        b = type(g).from_buffer_copy(g)
        b.lo[s], b.hi[s] = lo, hi
        bad.append(((s, lo, hi), b))
    return bad


class _Live:
    """one live context of a geometry at N = 1,000, its grids A and B (every sampler after every step) and one step"""

    def __init__(self, geom):
        self.geom = geom
        if geom == "temp":
            from argon_monte_carlo_amd.energised import SurfaceEnergies, device_rng_config
            from argon_monte_carlo_amd.engine import EnergisedEngine
            p, c = PR.pore_params(n=1_000, energised=True)
            p.reserved0 |= 1
            energies = SurfaceEnergies(c)
            p.E_cold, p.E_hot = energies.cold, energies.hot
            self.engine = EnergisedEngine(p)
            self.engine.upload(*IC.pore_ic(p, c, 23))
            cfg = device_rng_config(c, 11)
            self.step = lambda: self.engine.temp_timestep_device(c["dt"], cfg)
        else:
            from argon_monte_carlo_amd.engine import Engine
            p, c = PR.cube_params_for_n(1_000) if geom == "cube" else PR.pore_params(n=1_000)
            self.engine = Engine(p)
            self.engine.upload(*(IC.cube_ic if geom == "cube" else IC.pore_ic)(p, c, 11))
            self.step = lambda: self.engine.timestep(c["dt"])
        self.names = NAMES + ("free_paths",) + (("surfaces",) if geom == "temp" else ())
        self.grids = {label: _grids(geom, p, label) for label in "AB"}

    def config(self, name, label):
        _config(self.engine, name, None if label is None else self.grids[label][name], (1, 0))

    def sample(self, name):
        """one sample: the sampler's call, or a step for the two that sample the steps"""
        if name in ("free_paths", "surfaces"):
            self.step()
        else:
            getattr(self.engine, PREFIX[name] + "_sample")()
        return _read(self.engine, name)


@pytest.mark.parametrize("geom", ["cube", "pore", "temp"])
def test_a_sampler_gives_back_what_it_allocated(geom):
    """Free device memory against a tolerance of megabytes cannot see a buffer of four words that a *_free list has forgotten;
    the number of objects the context owns can."""
    live = _Live(geom)
    e = live.engine
    live.step()                             # (the step's own work spaces are built before the first reading)
    e.download()
    for name in live.names:
        base = e.owned_count()
        assert base > 10
        live.config(name, "A")
        a_config = e.owned_count()
        first = live.sample(name)
        a_sample = e.owned_count()
        assert a_config > base and first["counters"][N_SAMPLES.get(name, 0)] == 1, (name, first["counters"])
        live.config(name, "B")
        assert e.owned_count() == a_config, name            # the grid's size changes the buffers' sizes, not their number
        second = live.sample(name)
        assert e.owned_count() == a_sample, name
        assert second["totals"].shape != first["totals"].shape, name
        # an invalid grid leaves the count and the old configuration untouched
        good = bytes(getattr(e, GRID_ATTR[name]))
        for what, bad in _mutations(name, getattr(e, GRID_ATTR[name])):
            with pytest.raises(ArgonMCError) as err:
                getattr(e, PREFIX[name] + "_config")(bad)
            assert err.value.code == -1, (name, what)
            assert e.owned_count() == a_sample and bytes(getattr(e, GRID_ATTR[name])) == good, (name, what)
        again = live.sample(name)
        assert again["totals"].shape == second["totals"].shape and e.owned_count() == a_sample, name
        assert again["counters"][N_SAMPLES.get(name, 0)] == 2, (name, again["counters"])
        live.config(name, None)
        assert e.owned_count() == base, (name, e.owned_count(), base)
        live.config(name, None)             # (off twice: nothing to give back)
        assert e.owned_count() == base, name
    e.close()


@pytest.mark.parametrize("geom", ["cube", "pore", "temp"])
def test_all_samplers_at_once_give_back_what_they_allocated(geom):
    live = _Live(geom)
    e = live.engine
    live.step()
    e.download()
    base = e.owned_count()
    for name in live.names:
        live.config(name, "A")
    live.step()
    live.step()
    everything = e.owned_count()
    assert everything >= base + len(live.names)
    reads = {name: _read(e, name) for name in live.names}
    assert all(r["counters"][N_SAMPLES.get(name, 0)] == 2 for name, r in reads.items()), {k: r["counters"] for k, r in reads.items()}
    for name in reversed(live.names):       # reconfigured in another order, every grid of another size
        live.config(name, "B")
    live.step()
    assert e.owned_count() == everything
    order = [live.names[k] for k in (5, 0, 6, 4, 1, 3, 2)] + list(live.names[7:])
    assert sorted(order) == sorted(live.names)
    counts = []
    for name in order:                      # torn down in a third order: every one gives something back
        live.config(name, None)
        counts.append(e.owned_count())
    assert all(b < a for a, b in zip([everything] + counts, counts)), counts
    assert counts[-1] == base, (counts, base)
    live.step()                             # the context steps on without them
    assert e.owned_count() == base
    e.close()


def test_odd_count_all_samplers_after_every_step():
    """N = 4,099 (the walk's unpaired tail in every sampler at once), every sampler after every step of a short run."""
    from argon_monte_carlo_amd.sim import Simulation
    sim = Simulation("pore", n=ODD_N)
    sim.set_state(*IC.pore_ic(sim.params, sim.consts, 11))
    twin = Simulation("pore", n=ODD_N)
    twin.set_state(*IC.pore_ic(twin.params, twin.consts, 11))
    grids = _grids("pore", sim.params)
    _configure(sim.engine, grids, mix=EVERY_STEP, mfp=False)
    sim.run(3)
    states, records = [], []
    for _ in range(3):
        twin.timestep(collect_paths=False)
        records.append(twin.engine.drain_paths(sort=False))
        states.append(twin.engine.download())
    twin.close()
    _TRACE["odd"] = dict(states=states, records=records)
    for name in NAMES + ("free_paths",):
        want = _mirror("odd", name, grids[name], [1, 2, 3])
        _same(_read(sim.engine, name), want, name)
        assert name == "free_paths" or want["totals"].any(), name
    sim.close()
