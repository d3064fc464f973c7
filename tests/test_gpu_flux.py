"""GPU (-m gpu): sampled fluxes (include/argonmc_flux.h).  The device's integer totals must equal the NumPy + Python-int
reference (tests/flux_ref.py) on the downloaded states bit for bit, whatever the launch configuration or the way the steps were
driven, and sampling must change nothing else.  What the fluxes share with the other streaming samplers — two ranks, odd index
ranges, sampling changes nothing else — is in tests/test_gpu_sampler_protocol.py, and the body of run(k) against k timesteps in
tests/sampler_protocol.py."""
from fractions import Fraction

import numpy as np
import pytest

from argon_monte_carlo_amd import fields as FL
from argon_monte_carlo_amd import fluxes as FX
from argon_monte_carlo_amd import ic as IC
from argon_monte_carlo_amd import params as PR
from tests import fields_ref as FREF
from tests import sampler_protocol as SP
from tests.sampler_protocol import N
from tests.sampler_protocol import FluxMirror as Totals
from tests.sampler_protocol import make_sim as _sim

pytestmark = pytest.mark.gpu

_grid = SP.FLUXES.grids


# ---- 1. the totals equal the reference on the downloaded states -----------------------------------------------------------
@pytest.mark.parametrize("kind,n,which", [("cube", 1_000, "default"), ("cube", 1_000, "one"), ("cube", 1_000, "1024"),
                                          ("pore", 20_000, "default"), ("pore", 20_000, "one"), ("pore", 20_000, "cart")])
def test_totals_equal_reference_after_timesteps(kind, n, which):
    sim = _sim(kind, n)
    sim.enable_fluxes(_grid(kind, sim.params, which))
    g = sim.engine.flux_grid
    if which == "1024" or (kind, which) == ("pore", "default"):
        assert FX.grid_bins(g) == 1024  # the whole table in LDS
    ref = Totals(g)
    sim.fluxes_sample()                 # straight after the upload
    ref.add_state(sim.engine.download())
    for _ in range(3):
        sim.timestep()
        sim.fluxes_sample()             # the cube's sweep results are still deferred here: read through the slot arrays
        ref.add_state(sim.engine.download())
    tot = FX.words_to_ints(ref.check(sim.engine))
    assert sum(int(v) for v in tot[:, 0, 0]) + ref.n_outside == 4 * n
    assert not any(int(v) for v in tot[:, 1, 0])                            # the reserved slot is never added to
    assert any(int(v) for v in tot[:, 1, 1]) and any(int(v) for v in tot[:, 1, 6])
    f = sim.fluxes()
    full = f["count"] >= 2
    assert np.isfinite(f["heat_flux"][full]).all() and np.isfinite(f["pressure_tensor"][full]).all() and np.isnan(f["pressure"][~full]).all()
    sim.close()


# ---- 2. run(k) equals k timesteps, for any number of workgroups and in an overlapped run -----------------------------------
@pytest.mark.parametrize("kind,which,overlap,blocks", [
    ("cube", "default", None, None), ("pore", "default", None, None), ("cube", "default", "1", None), ("pore", "default", "1", None),
    ("cube", "9", None, "1"), ("pore", "9", None, "17"), ("cube", "9", None, "33"),
    ("pore", "10", None, "1"), ("cube", "10", None, "17"), ("pore", "10", None, "33")])
def test_run_equals_timesteps_and_reference(kind, which, overlap, blocks, monkeypatch):
    """9 bins: 2 * 63 sums + the outside column = 127 columns, one lane short of two workgroups of the reduce; 10 bins: 141, a
    third one with thirteen live lanes.  1, 17 and 33 slab rows: below, one above and two above a multiple of its sixteen waves."""
    SP.check_run(SP.FLUXES, monkeypatch, kind, which, overlap, blocks)


# ---- 3. row A against the fields ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["cube", "pore"])
def test_row_a_equals_the_fields_totals(kind):
    sim = _sim(kind, N, seed=3)
    sim.enable_fluxes(every=2)
    g = sim.engine.flux_grid
    sim.enable_fields(FL.make_grid(g.kind, (g.n1, g.n2, g.n3)[:3 if g.kind == FL.AMC_FIELDS_CARTESIAN else 2], list(g.lo), list(g.hi)), every=2)
    sim.run(6)
    f_tot, f_ns, f_no = sim.engine.fields_read()
    tot, ns, no = sim.engine.flux_read()
    assert (ns, no) == (f_ns, f_no) and ns == 3
    assert np.array_equal(tot[:, 0], f_tot) and f_tot.any() and tot[:, 1, 1:].any() and not tot[:, 1, 0].any()
    sim.close()


# ---- 5. a crafted state with a closed form -------------------------------------------------------------------------------------
def test_eight_crafted_particles_give_the_closed_form_stress_and_heat_flux():
    from argon_monte_carlo_amd.sim import Simulation
    sim = Simulation("pore", n=8)
    p = sim.params
    # multiples of 8 m/s: every quantised value is exact, so derive must return the exact central moments, rounded once
    vel = np.array([[8, 16, 24], [8, 16, -8], [-16, 40, 32], [24, -8, 0], [-40, 8, 16], [64, -24, 8], [0, 0, -48], [16, 32, 8]], dtype=np.float64)
    x = np.linspace(-0.3, 0.3, 8) * p.R_oa
    sim.set_state(x, 0.5 * x, np.full(8, 0.5 * p.H), *vel.T)
    sim.enable_fluxes(FX.make_grid("cartesian", (1, 1, 1), (-p.R_oa, -p.R_oa, 0.0), (p.R_oa, p.R_oa, p.H)))
    sim.fluxes_sample()
    f = sim.fluxes()
    assert f["count"].tolist() == [8] and f["n_samples"] == 1 and f["n_outside"] == 0
    fr = [[Fraction(int(k)) for k in c] for c in vel]
    u = [sum(c[a] for c in fr) / 8 for a in range(3)]
    Cs = [[c[a] - u[a] for a in range(3)] for c in fr]
    P = [[sum(C[a] * C[b] for C in Cs) / 8 for b in range(3)] for a in range(3)]
    q = [sum((C[0] ** 2 + C[1] ** 2 + C[2] ** 2) * C[a] for C in Cs) / 8 for a in range(3)]
    F = [sum((c[0] ** 2 + c[1] ** 2 + c[2] ** 2) * c[a] for c in fr) / 8 for a in range(3)]
    assert all(v != 0 for v in u + q + P[0] + P[1] + P[2])
    nd, m = f["number_density"][0], float(p.argon_mass)
    assert nd == 8 / (1 * f["bin_volume"][0])
    assert f["velocity"][0].tolist() == [float(v) for v in u]
    assert f["pressure_tensor"][0].tolist() == [[nd * m * float(P[a][b]) for b in range(3)] for a in range(3)]
    assert f["heat_flux"][0].tolist() == [nd * m / 2 * float(q[a]) for a in range(3)]
    assert f["energy_flux"][0].tolist() == [nd * m / 2 * float(F[a]) for a in range(3)]
    assert f["pressure"][0] == (f["pressure_tensor"][0, 0, 0] + f["pressure_tensor"][0, 1, 1] + f["pressure_tensor"][0, 2, 2]) / 3
    assert f["T"][0] == f["pressure"][0] / (nd * FX.boltzmann_constant(p))
    sim.close()


# ---- 6. the quantisers' range is checked, not wrapped ------------------------------------------------------------------------
def test_range_edge_is_reported_with_its_index_and_the_value_below_is_summed():
    from argon_monte_carlo_amd._lib import ArgonMCError
    from argon_monte_carlo_amd.sim import Simulation
    sim = Simulation("cube", n=1000)
    x, y, z, vx, vy, vz = IC.cube_ic(sim.params, sim.consts, 7)
    vx, vz = vx.copy(), vz.copy()
    top = float(np.nextafter(2.0 ** 14, 0))
    vx[417], vz[600], vz[601] = 2.0 ** 14, -(2.0 ** 14), top
    sim.set_state(x, y, z, vx, vy, vz)
    sim.enable_fluxes()
    sim.fluxes_sample()
    with pytest.raises(ArgonMCError) as e:
        sim.engine.flux_read()
    assert e.value.code == -4 and "particle 417 " in str(e.value)
    sim.fluxes_sample()                 # nothing is added while the error stands
    with pytest.raises(ArgonMCError):
        sim.engine.flux_read()
    sim.fluxes_reset()
    tot, ns, no = sim.engine.flux_read()
    assert ns == 0 and no == 0 and not tot.any()
    # the largest magnitude in range, in every component of two particles, is summed
    vx[417], vz[600] = -top, -top
    vx[601] = vy[601] = top
    sim.set_state(x, y, z, vx, vy, vz)
    sim.fluxes_sample()
    ref = Totals(sim.engine.flux_grid)
    ref.add(x, y, z, vx, vy, vz)
    tot = FX.words_to_ints(ref.check(sim.engine))
    assert max(abs(int(v)) for v in tot[:, 1, 4:].ravel()) >= 2 ** 37
    sim.close()


def test_calls_before_a_config_return_state_errors():
    from argon_monte_carlo_amd._lib import ArgonMCError
    sim = _sim("cube", 1000)
    for call in (sim.engine.lib.amc_flux_sample, sim.engine.lib.amc_flux_reset):
        assert call(sim.engine._ctx) == -6
    assert sim.engine.lib.amc_flux_read(sim.engine._ctx, None, None, None) == -6
    sim.enable_fluxes(every=1)
    sim.run(2)
    assert sim.engine.flux_read()[1] == 2
    sim.engine.reset_outputs()          # leaves the fluxes alone
    assert sim.engine.flux_read()[1] == 2
    sim.disable_fluxes()
    with pytest.raises(ArgonMCError) as e:
        sim.fluxes_sample()
    assert e.value.code == -6 and sim.engine.flux_grid is None
    g = FX.default_grid(sim.params)
    g.n1 = 1025                         # past the Python helper: the library refuses it too
    with pytest.raises(ArgonMCError) as e:
        sim.engine.flux_config(g)
    assert e.value.code == -1
    sim.close()


# ---- 8. checkpoints ------------------------------------------------------------------------------------------------------------
def test_checkpoint_resume_gives_the_same_totals(tmp_path):
    ck = str(tmp_path / "ck.npz")
    ref_tot = SP.uninterrupted(SP.FLUXES, 20_000)
    a = SP.checkpointed(SP.FLUXES, 20_000, ck)
    a.write_fluxes(str(tmp_path / "fluxes.npz"))
    a.close()
    z = np.load(str(tmp_path / "fluxes.npz"))
    assert z["totals"].shape == (1024, 2, 7, 2) and z["heat_flux"].shape == (1024, 3) and "edges_2" in z and int(z["n_samples"]) == 2
    tot = SP.resumed(SP.FLUXES, 20_000, ck, ref_tot)
    assert tot[0][:, 1].any()
    c = _sim("pore", 20_000)            # a checkpoint without fluxes: sampling is off in the resumed run
    c.run(1)
    c.save_checkpoint(str(tmp_path / "plain.npz"))
    c.enable_fluxes(every=1)
    c.load_checkpoint(str(tmp_path / "plain.npz"))
    assert c.engine.flux_grid is None
    c.close()


# ---- 9. the carry-add through the fluxes' load ----------------------------------------------------------------------------------
def test_flux_load_carry_and_borrow():
    """128-bit totals: loaded low words of 2^64 - 1 carry into the high word under a positive sum, low words of 0 borrow from it
    under a negative one; the result equals the exact Python-int sum, in both tables of the reduce."""
    from argon_monte_carlo_amd.engine import Engine
    n = 40
    k = np.arange(n)
    g = FX.make_grid("cartesian", (2, 1, 1), (-1.0e-7, -1.0e-7, 0.0), (1.0e-7, 1.0e-7, 1.0e-6))
    x, y, z = np.where(k % 2 == 0, -5.0e-8, 5.0e-8), np.zeros(n), np.full(n, 5.0e-7)
    state = (x, y, z, 300.0 + k, -(120.5 + 0.25 * k), -(77.0 + k))
    ref = Totals(g)
    ref.add(*state)
    sums = ref.sums
    assert ref.n_outside == 0 and (sums[:, 1, 1:] != 0).all() and (sums[:, 0] > 0)[:, [0, 1, 4, 5, 6]].all()
    assert (sums[:, 0, 2:4] < 0).all() and (sums[:, 1, [1, 2, 5, 6]] < 0).all() and (sums[:, 1, [3, 4]] > 0).all()
    loaded = np.empty(sums.shape, dtype=object)
    for idx in np.ndindex(sums.shape):
        loaded[idx] = (1 << 64) - 1 if sums[idx] > 0 else 0
    loaded[0, 0, 0] = (5 << 64) - 1                                  # high word already non-zero
    lw, ew = FX.ints_to_words(loaded), FX.ints_to_words(loaded + sums)
    carry, borrow = ew[..., 1] > lw[..., 1], ew[..., 1] < lw[..., 1]
    assert carry.sum() == (sums > 0).sum() == 2 * 7 and borrow.sum() == (sums < 0).sum() == 2 * 6
    p, _ = PR.pore_params(n=n)
    eng = Engine(p)
    eng.flux_config(g)
    eng.flux_load(lw, 9, 2)
    eng.upload(*state)
    eng.flux_sample()
    tot, ns, no = eng.flux_read()
    assert (ns, no) == (10, 2)
    assert np.array_equal(tot, ew), np.argwhere(tot != ew)[:5]
    eng.close()


# ---- 10. energised pore: host-RNG and device-RNG steps, and the host-free run ---------------------------------------------------
@pytest.mark.parametrize("device_rng", [False, True])
def test_energised_pore_totals_equal_reference(device_rng, tmp_path):
    sim, ref, tot = SP.energised_totals(SP.FLUXES, device_rng, every=2)
    assert ref.n_samples == 2 and tot[:, 1, 1:].any()
    f = sim.fluxes()
    assert np.isfinite(f["heat_flux"][f["count"] >= 2]).all()
    read, state = sim.engine.flux_read(), sim.engine.download()
    ck = str(tmp_path / "ck.npz")
    sim.save_checkpoint(ck)             # the energised class extends the base class's checkpoint: the fluxes travel with it
    sim.close()
    assert np.array_equal(np.load(ck)["flux_totals"], tot)
    if device_rng:                      # the host-free run takes the same samples as four single steps
        SP.host_free_run(SP.FLUXES, read, state, every=2)


# ---- 12. physics on a Maxwell start ---------------------------------------------------------------------------------------------
def test_maxwell_start_gives_isotropic_pressure_and_no_heat_flux():
    """Cube, n = 100,000, one sample on the default 8 x 8 x 8 grid (about 195 particles per bin).  Per bin, with the standard
    error of each mean taken from a host copy of that bin's velocities (C = c - <c>, se(w) = std(w) / sqrt(n)):
    pressure = nd m <|C|^2> / 3 within 6 se of nd k_B T; every off-diagonal P_ab = nd m <C_a C_b> and every heat-flux component
    q_a = nd m / 2 <|C|^2 C_a> within 6 se of zero.  6 sigma: about 2e-9 per value, times about 5e3 values."""
    n = 100_000
    sim = _sim("cube", n, seed=3)
    sim.enable_fluxes()
    sim.fluxes_sample()
    f = sim.fluxes()
    st = sim.engine.download()
    g = sim.engine.flux_grid
    b, c1, c2, c3 = FREF.bins_and_components(g, *(st[k] for k in ("x", "y", "z", "vx", "vy", "vz")))
    m = float(sim.params.argon_mass)
    kT = m * float(sim.consts["a_shape"]) ** 2           # the initial condition's k_B T (a_shape = sqrt(k_B T / m))
    assert f["n_outside"] == 0 and int(f["count"].sum()) == n and f["count"].min() >= 100
    worst = {"pressure": 0.0, "shear": 0.0, "heat": 0.0}
    for k in range(FX.grid_bins(g)):
        sel = b == k
        cnt = int(sel.sum())
        assert cnt == f["count"][k]
        c = np.stack([c1[sel], c2[sel], c3[sel]])
        C = c - c.mean(axis=1, keepdims=True)
        C2 = (C * C).sum(axis=0)
        nd = f["number_density"][k]

        def se(w):
            return float(np.std(w)) / np.sqrt(cnt)
        dev = abs(f["pressure"][k] - nd * kT) / (nd * m * se(C2 / 3))
        worst["pressure"] = max(worst["pressure"], dev)
        assert dev < 6, (k, "pressure", f["pressure"][k], nd * kT, dev)
        for a, c_ in ((0, 1), (0, 2), (1, 2)):
            dev = abs(f["pressure_tensor"][k, a, c_]) / (nd * m * se(C[a] * C[c_]))
            worst["shear"] = max(worst["shear"], dev)
            assert dev < 6 and f["pressure_tensor"][k, a, c_] == f["pressure_tensor"][k, c_, a], (k, a, c_, dev)
        for a in range(3):
            dev = abs(f["heat_flux"][k, a]) / (nd * m / 2 * se(C2 * C[a]))
            worst["heat"] = max(worst["heat"], dev)
            assert dev < 6, (k, "heat flux", a, f["heat_flux"][k, a], dev)
    print("largest deviations in standard errors:", worst)
    sim.close()
