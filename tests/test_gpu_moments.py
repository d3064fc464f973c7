"""GPU (-m gpu): the sampled fields and the sampled fluxes are two instances of one kernel template and one host core
(csrc/amc_fields.hip).  What the merge could get wrong and neither sampler's own tests pin: the shared LDS table at the
fields' full size, the two workspaces side by side on different grids and cadences, and the independence of their life
cycles.  N = 1,000 throughout; the references are tests/fields_ref.py and tests/flux_ref.py, bit for bit."""
import numpy as np
import pytest

from argon_monte_carlo_amd import _abi
from argon_monte_carlo_amd import fields as FL
from argon_monte_carlo_amd import fluxes as FX
from argon_monte_carlo_amd import ic as IC
from tests import fields_ref as FREF
from tests import flux_ref as XREF

pytestmark = pytest.mark.gpu

N = 1_000


def _sim(kind, seed=11):
    from argon_monte_carlo_amd.sim import Simulation
    sim = Simulation(kind, n=N)
    gen = IC.cube_ic if kind == "cube" else IC.pore_ic
    sim.set_state(*gen(sim.params, sim.consts, seed))
    return sim


class _FieldsTotals:
    """the fields' running totals over several samples: what amc_fields_read returns (XREF.Totals is the fluxes')"""

    def __init__(self, g):
        self.g, self.sums, self.n_samples, self.n_outside = g, np.empty((FL.grid_bins(g), 7), dtype=object), 0, 0
        self.sums[:] = 0

    def add_state(self, st):
        s, out = FREF.sample_state(self.g, st)
        self.sums = self.sums + s
        self.n_samples += 1
        self.n_outside += out

    def words(self):
        return FL.ints_to_words(self.sums)


def _equal(got, ref):
    """(totals, samples, outside) of a read against a reference's"""
    tot, ns, no = got
    assert (ns, no) == (ref.n_samples, ref.n_outside), (ns, no, ref.n_samples, ref.n_outside)
    want = ref.words()
    assert tot.shape == want.shape and np.array_equal(tot, want), np.argwhere(tot != want)[:5]


# ---- 1. the one LDS table at its full size, from the fields' side ------------------------------------------------------------
def test_fields_fill_the_whole_table_at_2048_bins_over_three_workgroups(monkeypatch):
    """Cartesian 16 x 16 x 8 over the cube: 2048 bins * 7 words, all of the table the two instances share (the fluxes reach it
    with 1024 bins * 14).  By count 1,000 particles are one workgroup: the knob makes the slab three rows."""
    monkeypatch.setenv("AMC_FIELDS_BLOCKS", "3")
    sim = _sim("cube")
    p = sim.params
    sim.enable_fields(FL.make_grid("cartesian", (16, 16, 8), (0, 0, 0), (p.cube_x, p.cube_y, p.cube_z)))
    g = sim.engine.field_grid
    assert FL.grid_bins(g) == 2048 == _abi.AMC_FIELDS_MAX_BINS == 2 * _abi.AMC_FLUX_MAX_BINS
    ref = _FieldsTotals(g)
    for _ in range(2):
        sim.timestep()
        sim.fields_sample()
        ref.add_state(sim.engine.download())
    _equal(sim.engine.fields_read(), ref)
    counts = ref.sums[:, 0]
    assert sum(counts) + ref.n_outside == 2 * N and ref.n_samples == 2
    assert sum(counts[1024:]) > 0        # the half of the table past the fluxes' bin limit is in use
    sim.close()


# ---- 2. both samplers on at once, different grids and cadences ----------------------------------------------------------------
STEPS, FIELDS_EVERY, FLUX_EVERY = 6, 2, 3


def _pore_grids(p):
    return (FL.make_grid("axisymmetric", (4, 8), (0, 0), (p.R_oa, p.H)),
            FX.make_grid("cartesian", (3, 2, 5), (-p.R_oa, -p.R_oa, 0.0), (p.R_oa, p.R_oa, p.H)))


def _pore_run(fields_on, flux_on):
    """six steps of the pore with the chosen samplers on their cadences -> (fields read, flux read, the state after every step,
    the two grids)"""
    sim = _sim("pore", seed=7)
    gf, gx = _pore_grids(sim.params)
    if fields_on:
        sim.enable_fields(gf, every=FIELDS_EVERY)
    if flux_on:
        sim.enable_fluxes(gx, every=FLUX_EVERY)
    states = []
    for _ in range(STEPS):
        sim.timestep()
        states.append(sim.engine.download())
    out = (sim.engine.fields_read() if fields_on else None, sim.engine.flux_read() if flux_on else None, states, (gf, gx))
    sim.close()
    return out


def test_both_samplers_at_once_equal_their_references_and_each_alone():
    """Fields axisymmetric 4 x 8 every 2, fluxes Cartesian 3 x 2 x 5 every 3: two workspaces that shared a slab, a meta word or
    a descriptor would show in the other's totals or counters."""
    f_both, x_both, states, (gf, gx) = _pore_run(True, True)
    f_ref, x_ref = _FieldsTotals(gf), XREF.Totals(gx)
    for s, st in enumerate(states, start=1):
        if s % FIELDS_EVERY == 0:
            f_ref.add_state(st)
        if s % FLUX_EVERY == 0:
            x_ref.add_state(st)
    assert (f_ref.n_samples, x_ref.n_samples) == (3, 2)
    _equal(f_both, f_ref)
    _equal(x_both, x_ref)
    assert f_both[0].shape == (32, 7, 2) and x_both[0].shape == (30, 2, 7, 2) and x_both[0][:, 1, 1:].any()
    f_alone, _, states_f, _ = _pore_run(True, False)
    _, x_alone, states_x, _ = _pore_run(False, True)
    for other in (states_f, states_x):
        assert all(np.array_equal(a[k], b[k]) for a, b in zip(states, other) for k in a)
    assert f_alone[1:] == f_both[1:] and np.array_equal(f_alone[0], f_both[0])
    assert x_alone[1:] == x_both[1:] and np.array_equal(x_alone[0], x_both[0])


# ---- 3. the life cycles are independent ----------------------------------------------------------------------------------------
def test_disable_enable_reset_and_the_error_word_touch_one_sampler_only():
    from argon_monte_carlo_amd._lib import ArgonMCError
    sim = _sim("cube", seed=5)
    p = sim.params
    x, y, z, vx, vy, vz = IC.cube_ic(p, sim.consts, 5)
    gf = FL.make_grid("cartesian", (4, 3, 2), (0, 0, 0), (p.cube_x, p.cube_y, p.cube_z))
    gx = FX.make_grid("cartesian", (2, 3, 4), (0, 0, 0), (0.5 * p.cube_x, p.cube_y, p.cube_z))      # the lower half in x
    sim.enable_fields(gf)
    sim.enable_fluxes(gx)
    sim.fields_sample()
    sim.fluxes_sample()
    st0 = sim.engine.download()
    f_ref, x_ref = _FieldsTotals(gf), XREF.Totals(gx)
    f_ref.add_state(st0)
    x_ref.add_state(st0)
    assert f_ref.n_outside == 0 and 0 < x_ref.n_outside < N
    f0, x0 = sim.engine.fields_read(), sim.engine.flux_read()
    _equal(f0, f_ref)
    _equal(x0, x_ref)
    # disable_fluxes() leaves the fields' read unchanged
    sim.disable_fluxes()
    assert sim.engine.flux_grid is None and sim.engine.lib.amc_flux_read(sim.engine._ctx, None, None, None) == -6
    f1 = sim.engine.fields_read()
    assert f1[1:] == f0[1:] and np.array_equal(f1[0], f0[0])
    # a later enable_fluxes() starts from zero
    sim.enable_fluxes(gx)
    tot, ns, no = sim.engine.flux_read()
    assert (ns, no) == (0, 0) and tot.shape == x0[0].shape and not tot.any()
    f1 = sim.engine.fields_read()
    assert f1[1:] == f0[1:] and np.array_equal(f1[0], f0[0])
    # fields_reset() does not touch the fluxes' totals
    sim.fluxes_sample()
    sim.fields_reset()
    tot, ns, no = sim.engine.fields_read()
    assert (ns, no) == (0, 0) and not tot.any()
    _equal(sim.engine.flux_read(), x_ref)                   # one sample of the same state since the fresh start
    # 2^14 on a particle outside the fluxes' grid and inside the fields': the fields' error word only
    bad = int(np.flatnonzero(x > 0.75 * p.cube_x)[7])
    vx = vx.copy()
    vx[bad] = 2.0 ** 14
    sim.set_state(x, y, z, vx, vy, vz)
    sim.fields_sample()
    sim.fluxes_sample()
    with pytest.raises(ArgonMCError) as e:
        sim.engine.fields_read()
    assert e.value.code == -4 and f"amc_fields: particle {bad} " in str(e.value) and "amc_fields_reset" in str(e.value)
    x_ref.add(x, y, z, vx, vy, vz)
    assert x_ref.n_samples == 2
    _equal(sim.engine.flux_read(), x_ref)
    sim.close()
