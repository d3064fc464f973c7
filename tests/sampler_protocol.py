"""What the GPU tests of the six streaming samplers share (tests/test_gpu_sampler_protocol.py and the samplers' own files):
the simulations they start, one worker for the two-rank tests, the stepwise reference of the run tests, computed once, and one
test record per sampler.  A record stands on the product's own ``samplers.Sampler`` (name, prefix, module, where the engine keeps
the grid) and adds what only the tests know: the workgroup knob, the named grids, a mirror with one face over the reference of
tests/<name>_ref.py, and per protocol test the values that test runs with.  The keyword arguments of ``enable_*`` (the
correlations' ``n_lags``) differ from test to test, so they stand with each test's values."""
import os
import random
from dataclasses import dataclass

import numpy as np

from argon_monte_carlo_amd import correlations as CO
from argon_monte_carlo_amd import distributions as VD
from argon_monte_carlo_amd import fields as FL
from argon_monte_carlo_amd import fluxes as FX
from argon_monte_carlo_amd import ic as IC
from argon_monte_carlo_amd import params as PR
from argon_monte_carlo_amd import samplers as S
from argon_monte_carlo_amd import transits as TR
from argon_monte_carlo_amd.totals import words_to_ints
from tests import corr_ref, fields_ref, flux_ref, pair_ref, transit_ref, vdf_ref
from tests.sampler_states import ODD_N, drifting_states

KEYS = ["x", "y", "z", "vx", "vy", "vz", "d", "dx", "dy", "dz", "flag"]
N = 20_011                              # odd: the unpaired tail; three workgroups


def make_sim(kind, n, seed=11):
    from argon_monte_carlo_amd.sim import Simulation
    sim = Simulation(kind, n=n)
    gen = IC.cube_ic if kind == "cube" else IC.pore_ic
    sim.set_state(*gen(sim.params, sim.consts, seed))
    return sim


def make_temp_sim(device_rng, n=20_000):
    """the energised pore, its walls' draws from the host's generators or from the device's (no sampler enabled)"""
    from argon_monte_carlo_amd.sim import TemperatureSimulation
    p, c = PR.pore_params(n=n, energised=True)
    sim = TemperatureSimulation(params=p, consts=c, np_rng=np.random.RandomState(3), py_rng=random.Random(3),
                                device_rng_seed=(7 if device_rng else None))
    sim.set_state(*IC.pore_ic(p, c, 13))
    return sim


# ---- the mirrors: add_state(downloaded state, lo, hi), add(x, y, z, vx, vy, vz), check(engine) -> the totals ----------------
class _FromState:
    def add_state(self, st, lo=0, hi=None):
        hi = len(st["x"]) if hi is None else hi
        self.add(*(st[k][lo:hi] for k in KEYS[:6]))


class FieldsMirror(_FromState):
    """Reference totals accumulated sample by sample (exact Python ints)."""

    def __init__(self, g):
        self.g, self.sums, self.outside, self.samples = g, np.zeros((FL.grid_bins(g), 7), dtype=object), 0, 0
        self.sums[:] = 0

    def add(self, *state):
        s, o = fields_ref.sample(self.g, *state)
        self.sums = self.sums + s
        self.outside += o
        self.samples += 1

    def check(self, engine):
        tot, ns, no = engine.fields_read()
        assert ns == self.samples and no == self.outside, (ns, self.samples, no, self.outside)
        ref = FL.ints_to_words(self.sums)
        assert np.array_equal(tot, ref), np.argwhere(tot != ref)[:5]
        return tot


class FluxMirror(flux_ref.Totals):
    def check(self, engine):
        tot, ns, no = engine.flux_read()
        assert (ns, no) == (self.n_samples, self.n_outside), (ns, no, self.n_samples, self.n_outside)
        want = self.words()
        assert tot.shape == want.shape and np.array_equal(tot, want), np.argwhere(tot != want)[:5]
        return tot


class CorrMirror(corr_ref.Window):
    def add(self, *state):
        corr_ref.Window.add(self, state)

    def add_state(self, st, lo=0, hi=None):
        self.add(*corr_ref.state6(st, lo, hi))

    def check(self, engine):
        tot, counters = engine.corr_read()
        assert counters == self.counters(), (counters, self.counters())
        ref = self.words()
        assert np.array_equal(tot, ref), np.argwhere(tot != ref)[:5]
        return tot


class VdfMirror(vdf_ref.Totals):
    def check(self, engine):
        tot, ns, no = engine.vdf_read()
        assert (ns, no) == (self.n_samples, self.n_outside), (ns, no, self.n_samples, self.n_outside)
        assert tot.shape == self.sums.shape and tot.dtype == np.int64 and np.array_equal(tot, self.sums), np.argwhere(tot != self.sums)[:5]
        vdf_ref.check_invariants(engine.vdf_grid, tot)
        return tot


class TransitMirror(_FromState, transit_ref.Mirror):
    """(built from the zones and the number of particles; check also compares the per-particle arrays, and returns the totals as
    Python ints)"""

    def add(self, *state):
        self.sample(*state[:3])

    def check(self, engine):
        tot, ns = engine.transit_read()
        want = self.words()
        assert ns == self.n_samples, (ns, self.n_samples)
        assert tot.shape == want.shape and tot.dtype == np.int64 and np.array_equal(tot, want), np.argwhere(tot != want)[:5]
        state, entry = engine.transit_state()
        assert np.array_equal(state, self.state), np.flatnonzero(state != self.state)[:5]
        for k in range(len(self.zones)):
            inside = ((self.state >> np.uint32(4 * k)) & np.uint32(3)) == 2
            assert np.array_equal(entry[k][inside], self.entry[k][inside]), k
        return words_to_ints(tot)


class PairMirror(pair_ref.Totals):
    """(add_state takes the whole state: [lo, hi) are the centres, everybody is a neighbour)"""

    def add(self, *state):
        self.add_state(dict(zip(KEYS[:6], state)))

    def check(self, engine):
        tot, ns, no, nu = engine.pair_read()
        assert (ns, no, nu) == (self.n_samples, self.n_outside, self.n_unfiled), ((ns, no, nu), self.read()[1:])
        assert tot.shape == self.sums.shape and tot.dtype == np.int64 and np.array_equal(tot, self.sums), np.argwhere(tot != self.sums)[:5]
        return tot


# ---- the named grids -----------------------------------------------------------------------------------------------------------
def _fields_grid(kind, params, which):
    if which == "default":
        return FL.default_grid(params)
    if which == "one":
        if kind == "cube":
            return FL.make_grid("cartesian", (1, 1, 1), (0, 0, 0), (params.cube_x, params.cube_y, params.cube_z))
        return FL.make_grid("axisymmetric", (1, 1), (0, 0), (params.R_oa, params.H))
    assert which == "cart"          # a Cartesian grid in the pore, over its bounding box
    return FL.make_grid("cartesian", (6, 6, 40), (-params.R_oa, -params.R_oa, 0.0), (params.R_oa, params.R_oa, params.H))


def _flux_grid(kind, p, which):
    if which == "default":
        return FX.default_grid(p)
    if which == "cart":                 # a Cartesian grid in the pore, over its bounding box
        return FX.make_grid("cartesian", (5, 5, 40), (-p.R_oa, -p.R_oa, 0.0), (p.R_oa, p.R_oa, p.H))
    n3 = {"one": (1, 1, 1), "1024": (16, 8, 8), "9": (9, 1, 1), "10": (5, 2, 1)}[which]
    if kind == "cube":
        return FX.make_grid("cartesian", n3, (0, 0, 0), (p.cube_x, p.cube_y, p.cube_z))
    return FX.make_grid("axisymmetric", (n3[1] * n3[2], n3[0]), (0, 0), (p.R_oa, p.H))


def _corr_grid(kind, params, which, n_lags):
    if which == "default":
        return CO.default_grid(params, n_lags=n_lags)
    if which == "one":
        if kind == "cube":
            return CO.make_grid("cartesian", (1, 1, 1), (0, 0, 0), (params.cube_x, params.cube_y, params.cube_z), n_lags=n_lags)
        return CO.make_grid("axisymmetric", (1, 1), (0, 0), (params.R_oa, params.H), n_lags=n_lags)
    assert which == "444" and kind == "cube"
    return CO.make_grid("cartesian", (4, 4, 4), (0, 0, 0), (params.cube_x, params.cube_y, params.cube_z), n_lags=n_lags)


# regions and histogram bins per named grid: W = regions * (4 H + 8) columns and the outside column make W + 1 slab columns
_VDF_SHAPES = {"one": ((1, 1, 1), 64), "exact": ((8, 8, 6), 14), "125": ((1, 1, 1), 29), "129": ((2, 2, 2), 2), "133": ((11, 1, 1), 1)}


def _vdf_grid(kind, p, which):
    if which == "default":
        return VD.default_grid(p)
    if which == "cart":                 # a Cartesian grid in the pore, over its bounding box
        return VD.make_grid("cartesian", (2, 2, 8), (-p.R_oa, -p.R_oa, 0.0), (p.R_oa, p.R_oa, p.H))
    if which == "half":                 # ... and over the half x >= 0 of it: the other half of the particles is outside
        return VD.make_grid("cartesian", (1, 2, 8), (0.0, -p.R_oa, 0.0), (p.R_oa, p.R_oa, p.H))
    n3, H = _VDF_SHAPES[which]
    if kind == "cube":
        return VD.make_grid("cartesian", n3, (0, 0, 0), (p.cube_x, p.cube_y, p.cube_z), hist_bins=H)
    return VD.make_grid("axisymmetric", (n3[2], n3[0] * n3[1]), (0, 0), (p.R_oa, p.H), hist_bins=H)


def vdf_slab_columns(g):
    return VD.grid_bins(g) * VD.columns(g.hist_bins) + 1


def thin_zones(p):
    """The pore moves an atom about 0.07 nm per step: zones thin enough for whole residences within a test — 0.5 nm and 2 nm
    at the lower mouth of the coated section, nested, and one abutting the floor z = 0."""
    return [(2, p.h_oa, p.h_oa + 0.5e-9), (2, p.h_oa, p.h_oa + 2e-9), (2, 0.0, 1e-9)]


def transit_zones(kind, p):
    return TR.zones(TR.default_grid(p)) if kind == "cube" else thin_zones(p)


def _transit_grid(kind, p, which=None):
    return TR.make_grid(transit_zones(kind, p))


def transit_classes(t, k):
    return [int(t[k, TR.class_column(e, x)]) for e in range(3) for x in range(2)]


def _transit_exits(t):
    return sum(sum(transit_classes(t, k)) for k in range(len(t)))


# ---- what only one sampler asserts at the end of a shared test ------------------------------------------------------------------
def _fields_odd(eng, m, tot, states, lo, hi):
    assert m.sums[:, 0].sum() + m.outside == 4 * (hi - lo)


def _flux_odd(eng, m, tot, states, lo, hi):
    assert sum(int(v) for v in FX.words_to_ints(tot)[:, 0, 0]) + m.n_outside == 3 * (hi - lo)


def _corr_odd(eng, m, tot, states, lo, hi):
    """n_lags = 2 and four samples: an origin, a lag, the lag-and-origin pass, a lag.  The origin arrays outside [lo, hi) stay zero."""
    tot = CO.words_to_ints(tot)
    assert m.counters() == (2, 4, m.n_outside, 2)
    assert all(any(int(v) != 0 for v in tot[:, lag, 1]) for lag in (1, 2))           # both lags saw displacements
    origin = eng.corr_origin()
    assert all(np.array_equal(o, a[lo:hi]) for o, a in zip(origin, states[2]))      # the origin stored by the third sample


def _vdf_odd(eng, m, tot, states, lo, hi):
    assert int(tot[:, 0].sum()) + m.n_outside == 3 * (hi - lo)


def _transit_odd(eng, m, t, states, lo, hi):
    zones = len(m.zones)
    assert all(int(t[k, 0:3].sum()) > 0 for k in range(zones)) and int(t[:, 0:2].sum()) > 0 and _transit_exits(t) > 0
    state, entry = eng.transit_state()
    assert state.shape == (hi - lo,) and entry.shape == (zones, hi - lo)


def _flux_ranks(ref, n):
    assert ref[0][:, 1].any()


def _corr_ranks(ref, n):
    assert ref[0][:, 2].any()


def _vdf_ranks(ref, n):
    assert int(ref[0][:, 0].sum()) + ref[2] == 3 * n


def _transit_ranks(ref, n):
    t = words_to_ints(ref[0])
    assert int(t[:, 0:3].sum()) > 0 and int(t[:, 4].sum()) > 0


def _transit_run_reference(t):
    assert _transit_exits(t) > 0


# ---- the reduce's cases: (params, grid, state) per shape, and what the shape must be ---------------------------------------------
def _reduce_state():
    p, (st,) = drifting_states(ODD_N, 1, seed=29)
    return p, st


def _fields_reduce(bins):
    """``bins`` bins over the lower half of the pore's box.  9 bins: 9 * 7 sums + the outside column = 64 columns, one full
    workgroup of the reduce; 10 bins: 71, a second one with seven live lanes."""
    p, st = _reduce_state()
    return p, FL.make_grid("cartesian", {9: (3, 3, 1), 10: (5, 2, 1)}[bins], (-p.R_oa, -p.R_oa, 0.0), (p.R_oa, p.R_oa, 0.5 * p.H)), st


def _fields_reduce_shape(bins, g, sums, outside):
    assert FL.grid_bins(g) == bins and bins * 7 + 1 == {9: 64, 10: 71}[bins] and outside > 0 and (sums[:, 0] > 0).all()


def _vdf_reduce(regions):
    """4 regions of H = 2: W = 4 * 16 = 64 totals columns, the last one lane 63 of the reduce's first workgroup, the outside column
    lane 0 of a second one; 5 regions of H = 1: W = 60, one partial workgroup."""
    p, st = _reduce_state()
    return p, VD.make_grid("cartesian", (regions, 1, 1), (-p.R_oa, -p.R_oa, 0.0), (p.R_oa, p.R_oa, 0.5 * p.H), hist_bins={4: 2, 5: 1}[regions]), st


def _vdf_reduce_shape(regions, g, sums, outside):
    assert vdf_slab_columns(g) - 1 == {4: 64, 5: 60}[regions] and outside > 0 and (sums[:, 0] > 0).all()


def _same(sums):
    return sums


# ---- the records -----------------------------------------------------------------------------------------------------------------
def _second(read):
    return read[1]


def _no_more(engine):
    return ()


@dataclass(frozen=True)
class Record:
    sampler: S.Sampler              # the product's record: name, prefix, module, grid_attr
    blocks: str                     # the environment's knob for the number of workgroups
    mirror: object                  # (grid, particles) -> the mirror
    grids: object = None            # (kind, params, which) -> a named grid
    samples: object = _second       # read -> the counters that the cadence decides, not the state
    more: object = _no_more         # engine -> further device state a run must reproduce
    # per protocol test (None: the sampler's own file has it, or nothing like it)
    invisible: dict = None          # n, enable: the keyword arguments, samples: after run(10) and ten timesteps
    ranks: dict = None              # every, enable, [grid: (kind, params) ->], dt: the derive takes it, samples: after six steps, [tail]
    odd: dict = None                # states, grid: params ->, tail
    run: dict = None                # n, steps, every, enable, grid: (kind, params, which) -> (None: the default), manual: the
    #                                 reference samples by hand, samples (the cases are in the samplers' files: check_run)
    reduce: dict = None             # shapes, case: shape -> (params, grid, state), ref: one sample's sums and counters,
    #                                 words: sums -> what a read returns, shape: the assertion on the case

    @property
    def name(self):
        return self.sampler.name

    def enable(self, sim, grid=None, **kw):
        getattr(sim, "enable_" + self.sampler.name)(grid, **kw)

    def config(self, engine, grid):
        getattr(engine, self.sampler.prefix + "_config")(grid)

    def sample(self, engine):
        getattr(engine, self.sampler.prefix + "_sample")()

    def read(self, engine):
        return getattr(engine, self.sampler.prefix + "_read")()

    def mirror_of(self, engine, n=None):
        return self.mirror(getattr(engine, self.sampler.grid_attr), n)

    def ranks_grid(self, kind, p):
        """the grid of the two-rank test: its own, or the default one with the test's cadence"""
        r = self.ranks
        return r["grid"](kind, p) if "grid" in r else self.sampler.module.default_grid(p, every=r["every"], **r["enable"])


def _no_grid(kind, p, which):
    return None


FIELDS = Record(
    S.FIELDS, "AMC_FIELDS_BLOCKS", lambda g, n: FieldsMirror(g), _fields_grid,
    invisible=dict(n=50_000, enable=dict(every=3), samples=6),           # steps 3, 6, 9 (inside run) and 12, 15, 18
    ranks=dict(every=2, enable={}, dt=False, samples=3),
    odd=dict(states=4, grid=FL.default_grid, tail=_fields_odd),
    run=dict(n=100_003, steps=7, every=2, enable=dict(every=2), grid=_no_grid, manual=False, samples=3),
    reduce=dict(shapes=(9, 10), case=_fields_reduce, ref=fields_ref.sample, words=FL.ints_to_words, shape=_fields_reduce_shape))

FLUXES = Record(
    S.FLUXES, "AMC_FLUX_BLOCKS", lambda g, n: FluxMirror(g), _flux_grid,
    invisible=dict(n=N, enable=dict(every=2), samples=10),
    ranks=dict(every=2, enable={}, dt=False, samples=3, tail=_flux_ranks),
    odd=dict(states=3, grid=FX.default_grid, tail=_flux_odd),
    run=dict(n=N, steps=7, every=2, enable=dict(every=2), grid=_flux_grid, manual=True, samples=3))

CORRELATIONS = Record(
    S.CORRELATIONS, "AMC_CORR_BLOCKS", lambda g, n: CorrMirror(g), _corr_grid,
    samples=lambda read: (read[1][0], read[1][1], read[1][3]),             # origins, samples, the window's position
    invisible=dict(n=N, enable=dict(every=2, n_lags=3), samples=(4, 10, 1)),      # steps 2, 4, ... 20: origins at 2, 8, 14, 20
    ranks=dict(every=2, enable=dict(n_lags=2), dt=True, samples=(2, 3, 1), tail=_corr_ranks),
    odd=dict(states=4, grid=lambda p: CO.default_grid(p, n_lags=2), tail=_corr_odd),
    run=dict(n=N, steps=7, every=2, enable=dict(every=2, n_lags=2), grid=_no_grid, manual=False,
             samples=(2, 3, 1)))                                                    # steps 2 (origin), 4 (lag 1), 6 (lag 2 + origin)

DISTRIBUTIONS = Record(
    S.DISTRIBUTIONS, "AMC_VDF_BLOCKS", lambda g, n: VdfMirror(g), _vdf_grid,
    invisible=dict(n=N, enable=dict(every=2), samples=10),
    ranks=dict(every=2, enable={}, dt=False, samples=3, tail=_vdf_ranks),
    odd=dict(states=3, grid=VD.default_grid, tail=_vdf_odd),
    run=dict(n=N, steps=7, every=2, enable=dict(every=2), grid=_vdf_grid, manual=True, samples=3,
             columns=(vdf_slab_columns, {"125": 125, "129": 129, "133": 133})),
    reduce=dict(shapes=(4, 5), case=_vdf_reduce, ref=vdf_ref.sample, words=_same, shape=_vdf_reduce_shape))

TRANSITS = Record(
    S.TRANSITS, "AMC_TRANSIT_BLOCKS", lambda g, n: TransitMirror(TR.zones(g), n), _transit_grid,
    more=lambda engine: (engine.transit_state()[0],),
    invisible=dict(n=N, enable=dict(every=2), samples=10),
    ranks=dict(every=1, enable={}, grid=_transit_grid, dt=True, samples=6, tail=_transit_ranks),
    # (uploads do not restart tracking: every sample follows an upload)
    odd=dict(states=24, grid=lambda p: TR.make_grid(thin_zones(p) + [(0, -2e-9, 2e-9), (1, 0.0, 5e-9)], every=0), tail=_transit_odd),
    run=dict(n=N, steps=12, every=1, enable={}, grid=_transit_grid, manual=False, samples=12, reference=_transit_run_reference))

# (the pairs share the mirror and the simulations; every test of theirs has a body of its own)
PAIRS = Record(S.PAIRS, "AMC_PAIR_BLOCKS", lambda g, n: PairMirror(g))

RECORDS = {r.name: r for r in (FIELDS, FLUXES, CORRELATIONS, DISTRIBUTIONS, TRANSITS, PAIRS)}


def having(test):
    """the records of the samplers that have the protocol test ``test``"""
    return [r for r in RECORDS.values() if getattr(r, test) is not None]


# ---- two ranks on one GPU: the child processes' body ---------------------------------------------------------------------------
def sampler_worker(rank, world, port, sampler_name, kind, n, steps, every, q):
    import torch.distributed as dist
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        try:
            from argon_monte_carlo_amd.dist import ShardedSimulation
            from tests.test_gpu_dist import _case
            rec = RECORDS[sampler_name]
            p, c, init = _case(kind, n)
            sim = ShardedSimulation(p, rank, world, backend="gloo")
            sim.upload(*init)
            rec.enable(sim, rec.ranks["grid"](kind, p) if "grid" in rec.ranks else None, every=every, **rec.ranks["enable"])
            sim.run(c["dt"], steps)
            d = getattr(sim, rec.name)(**({"dt": c["dt"]} if rec.ranks["dt"] else {}))
            if rank == 0:
                q.put(("ok", rec.sampler.join_read(d["totals"], (), [d[k] for k in rec.sampler.counters])))
        finally:
            dist.destroy_process_group()
    except BaseException as e:
        import traceback
        q.put(("error", f"rank {rank}: {e!r}\n{traceback.format_exc()}"))
        raise


# ---- run(k) against k timesteps: the stepwise side, against the mirror, once per (sampler, geometry, grid) ----------------------
_RUN_REF = {}


def run_reference(rec, kind, which):
    """timesteps with the cadence (or with samples by hand) against the mirror: (the read, rec.more, the final state)"""
    key = (rec.name, kind, which)
    if key not in _RUN_REF:
        r = rec.run
        sim = make_sim(kind, r["n"])
        rec.enable(sim, r["grid"](kind, sim.params, which), **({} if r["manual"] else r["enable"]))
        m = rec.mirror_of(sim.engine, r["n"])
        for s in range(1, r["steps"] + 1):
            sim.timestep()
            if s % r["every"] == 0:
                if r["manual"]:
                    getattr(sim, rec.name + "_sample")()
                m.add_state(sim.engine.download())
        tot = m.check(sim.engine)
        if "reference" in r:
            r["reference"](tot)
        _RUN_REF[key] = (rec.read(sim.engine), rec.more(sim.engine), sim.engine.download())
        sim.close()
    return _RUN_REF[key]


def check_run(rec, monkeypatch, kind, which=None, overlap=None, blocks=None, mfp=False):
    """run(steps) equals the stepwise reference — totals, counters, rec.more and the final state — in an overlapped run
    (AMC_OVERLAP), with ``blocks`` workgroups, beside the free paths.  The samplers' files call it with their own cases."""
    r = rec.run
    ref_read, ref_more, ref_state = run_reference(rec, kind, which)
    if overlap is not None:
        monkeypatch.setenv("AMC_OVERLAP", overlap)
    if blocks is not None:
        monkeypatch.setenv(rec.blocks, blocks)
    sim = make_sim(kind, r["n"])
    if mfp:
        sim.enable_free_paths()
    rec.enable(sim, r["grid"](kind, sim.params, which), **r["enable"])
    if which in r.get("columns", (None, ()))[1]:
        assert r["columns"][0](getattr(sim.engine, rec.sampler.grid_attr)) == r["columns"][1][which]
    sim.run(r["steps"])
    got = rec.read(sim.engine)
    assert got[1:] == ref_read[1:] and rec.samples(got) == r["samples"]
    assert np.array_equal(got[0], ref_read[0]), np.argwhere(got[0] != ref_read[0])[:5]
    assert all(np.array_equal(a, b) for a, b in zip(rec.more(sim.engine), ref_more, strict=True))
    st = sim.engine.download()
    for k in KEYS:
        assert np.array_equal(st[k], ref_state[k]), k
    sim.close()


# ---- the reduce at its shapes: one sample's reference, once per (sampler, shape) --------------------------------------------------
_REDUCE_REF = {}


def reduce_reference(rec, shape):
    """(params, grid, state, the reference's sums of one sample, its counters: outside[, unfiled])"""
    if (rec.name, shape) not in _REDUCE_REF:
        p, g, st = rec.reduce["case"](shape)
        _REDUCE_REF[(rec.name, shape)] = (p, g, st) + tuple(rec.reduce["ref"](g, *st))
    return _REDUCE_REF[(rec.name, shape)]


# ---- the energised pore and the checkpoint: the part every sampler's test has; what a sampler adds stays in its file --------------
def energised_totals(rec, device_rng, **enable):
    """Four steps of the energised pore with the sampler's cadence, the mirror on the downloaded state of every sampled step:
    (the simulation, still open; the mirror; the checked totals)"""
    sim = make_temp_sim(device_rng)
    rec.enable(sim, **enable)
    m = rec.mirror_of(sim.engine)
    for s in range(1, 5):
        sim.timestep()
        if s % enable["every"] == 0:
            m.add_state(sim.engine.download())
    return sim, m, m.check(sim.engine)


def host_free_run(rec, read, state, **enable):
    """run(4) with the device's generators takes the same samples as the four single steps that read ``read`` and left ``state``"""
    run = make_temp_sim(True)
    rec.enable(run, **enable)
    run.run(4)
    got = rec.read(run.engine)
    assert got[1:] == read[1:] and np.array_equal(got[0], read[0])
    st = run.engine.download()
    for k in KEYS:
        assert np.array_equal(st[k], state[k]), k
    run.close()


def uninterrupted(rec, n):
    """run(7) and run(8) with a sample after every third step: the read"""
    ref = make_sim("pore", n, seed=4)
    rec.enable(ref, every=3)
    ref.run(7)
    ref.run(8)
    out = rec.read(ref.engine)
    ref.close()
    return out


def checkpointed(rec, n, path):
    """run(7) and a checkpoint at ``path``: the simulation, still open"""
    a = make_sim("pore", n, seed=4)
    rec.enable(a, every=3)
    a.run(7)
    a.save_checkpoint(path)
    return a


def resumed(rec, n, path, ref):
    """A new simulation from the checkpoint — it restores the grid, the totals and the cadence (steps 9, 12, 15 still to come) —
    runs the eight steps and reads what the uninterrupted run read: the read"""
    from argon_monte_carlo_amd.sim import Simulation
    b = Simulation("pore", n=n)
    b.load_checkpoint(path)
    b.run(8)
    tot = rec.read(b.engine)
    assert tot[1] == ref[1] == 5 and tot[2] == ref[2]
    assert np.array_equal(tot[0], ref[0])
    b.close()
    return tot
