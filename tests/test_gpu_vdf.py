"""GPU (-m gpu): sampled velocity distributions (include/argonmc_vdf.h).  The device's integer counts must equal the NumPy
reference (tests/vdf_ref.py) on the downloaded states bit for bit, whatever the launch configuration or the way the steps were
driven, and sampling must change nothing else.  What the distributions share with the other streaming samplers — two ranks, odd
index ranges, the reduce's shapes, sampling changes nothing else — is in tests/test_gpu_sampler_protocol.py, and the body of
run(k) against k timesteps in tests/sampler_protocol.py."""
import math

import numpy as np
import pytest

from argon_monte_carlo_amd import distributions as VD
from argon_monte_carlo_amd import fields as FL
from argon_monte_carlo_amd import ic as IC
from argon_monte_carlo_amd import params as PR
from tests import sampler_protocol as SP
from tests import vdf_ref as REF
from tests.sampler_protocol import VdfMirror as Totals
from tests.sampler_protocol import make_sim as _sim
from tests.sampler_protocol import vdf_slab_columns as _slab_columns

pytestmark = pytest.mark.gpu

_grid = SP.DISTRIBUTIONS.grids


# ---- 1. the totals equal the reference on the downloaded states -----------------------------------------------------------
@pytest.mark.parametrize("kind,n,which", [("cube", 1_000, "default"), ("cube", 1_000, "one"), ("cube", 1_000, "exact"),
                                          ("pore", 20_000, "default"), ("pore", 20_000, "one"), ("pore", 20_000, "cart"),
                                          ("pore", 20_000, "half")])
def test_totals_equal_reference_after_timesteps(kind, n, which):
    """(The pore's bounding box holds every particle — R_oa is its largest radius — so the grid over it counts nobody outside; the
    grid over half of it does.)"""
    sim = _sim(kind, n)
    sim.enable_distributions(_grid(kind, sim.params, which))
    g = sim.engine.vdf_grid
    if which == "exact":
        assert _slab_columns(g) - 1 == 24_576       # the whole table in LDS
    axes = 3 if g.kind == FL.AMC_FIELDS_CARTESIAN else 2
    sim.enable_fields(FL.make_grid(g.kind, (g.n1, g.n2, g.n3)[:axes], list(g.lo)[:axes], list(g.hi)[:axes]))      # the same regions
    ref = Totals(g)
    sim.distributions_sample()          # straight after the upload
    sim.fields_sample()
    ref.add_state(sim.engine.download())
    for _ in range(3):
        sim.timestep()
        sim.distributions_sample()      # the cube's sweep results are still deferred here: read through the slot arrays
        sim.fields_sample()
        ref.add_state(sim.engine.download())
    tot = ref.check(sim.engine)
    assert int(tot[:, 0].sum()) + ref.n_outside == 4 * n
    assert (ref.n_outside > 0) == (which == "half")
    f_tot, f_ns, f_no = sim.engine.fields_read()
    assert (f_ns, f_no) == (4, ref.n_outside) and np.array_equal(f_tot[:, 0, 0], tot[:, 0]) and not f_tot[:, 0, 1].any()
    d = sim.distributions()
    full = d["count"] >= 1
    assert np.isfinite(d["pdf"][full]).all() and np.isnan(d["pdf"][~full]).all() and d["n_samples"] == 4
    sim.close()


# ---- 2. run(k) equals k timesteps, for any number of workgroups and in an overlapped run -----------------------------------
@pytest.mark.parametrize("kind,which,overlap,blocks", [
    ("cube", "default", None, None), ("pore", "default", None, None), ("cube", "default", "1", None), ("pore", "default", "1", None),
    ("cube", "125", None, "1"), ("pore", "125", None, "17"), ("cube", "129", None, "33"),
    ("pore", "129", None, "1"), ("cube", "133", None, "17"), ("pore", "133", None, "33")])
def test_run_equals_timesteps_and_reference(kind, which, overlap, blocks, monkeypatch):
    """The reduce takes 64 slab columns per workgroup.  A slab row has regions * (4 H + 8) + 1 columns, which is 1 modulo 4, so
    127 and 128 columns do not exist; the sizes around the boundary between two and three workgroups are 125 (one region, H = 29:
    three lanes short of two full workgroups), 129 (8 regions, H = 2: a third workgroup with one live lane) and 133 (11 regions,
    H = 1, C = 12: five live lanes); the shared body asserts each.  1, 17 and 33 slab rows: below, one above and two above a
    multiple of its sixteen waves."""
    SP.check_run(SP.DISTRIBUTIONS, monkeypatch, kind, which, overlap, blocks)


# ---- 4. crafted edges ---------------------------------------------------------------------------------------------------------------
def test_crafted_edge_values_land_in_the_documented_columns():
    """One region, H = 64, v_max = 2048: component bins of 64 m/s, speed bins of 32 m/s.  The expected table is written out by hand.
    nextafter(64, 0) is counted in bin 33, not 32: the rule bins floor((c + v_max) / w), and 63.99999999999999 + 2048 rounds to
    2112 in IEEE double (the header says so); every other edge lands where exact arithmetic puts it."""
    from argon_monte_carlo_amd.sim import Simulation
    n = 40
    sim = Simulation("pore", n=n)
    p = sim.params
    up, dn = float(np.nextafter(2048.0, math.inf)), float(np.nextafter(-2048.0, -math.inf))
    b64 = float(np.nextafter(64.0, 0.0))
    v = np.zeros((n, 3))
    v[0] = (-2048.0, 0, 0)              # c1 bin 0;       speed exactly 2048: bin 63
    v[1] = (dn, 0, 0)                   # c1 under;       speed over
    v[2] = (2048.0, 0, 0)               # c1 bin 63;      speed exactly 2048: bin 63
    v[3] = (up, 0, 0)                   # c1 over;        speed just above 2048: over
    v[4] = (0.0, -0.0, 0.0)             # all bin 32;     speed 0: bin 0
    v[5] = (0, -64.0, 0)                # c2 bin 31;      speed 64: bin 2
    v[6] = (0, b64, 0)                  # c2 bin 33;      speed just below 64: bin 1
    v[7] = (0, 0, 2048.0)               # c3 bin 63;      speed bin 63
    v[8] = (0, 0, dn)                   # c3 under;       speed over
    v[9] = (0, 0, -64.0)                # c3 bin 31;      speed bin 2
    v[10] = (2048.0, 0, 1.0)            # c1 bin 63, c3 bin 32; speed sqrt(2048^2 + 1) > 2048: over, every component in range
    v[11] = (1200.0, 1200.0, 1200.0)    # all bin 50;     speed 2078.5: over
    x = np.linspace(-0.3, 0.3, n) * p.R_oa
    state = (x, 0.5 * x, np.full(n, 0.5 * p.H), v[:, 0].copy(), v[:, 1].copy(), v[:, 2].copy())
    sim.set_state(*state)
    g = VD.make_grid("cartesian", (1, 1, 1), (-p.R_oa, -p.R_oa, 0.0), (p.R_oa, p.R_oa, p.H), hist_bins=64, v_max=2048.0)
    sim.enable_distributions(g)
    sim.distributions_sample()
    tot, ns, no = sim.engine.vdf_read()
    want = np.zeros((1, 264), dtype=np.int64)
    want[0, 0] = 40

    def comp(e, under=0, over=0, **bins):
        base = 1 + 66 * e
        want[0, base], want[0, base + 65] = under, over
        for k, cnt in bins.items():
            want[0, base + 1 + int(k[1:])] = cnt
    comp(0, under=1, over=1, b0=1, b63=2, b50=1, b32=34)
    comp(1, b31=1, b33=1, b50=1, b32=37)
    comp(2, under=1, b63=1, b31=1, b50=1, b32=36)
    for k, cnt in {63: 3, 64: 5, 2: 2, 1: 1, 0: 29}.items():       # the speed: h[0..64), over at 64
        want[0, 199 + k] = cnt
    assert (ns, no) == (1, 0) and np.array_equal(tot, want), np.argwhere(tot != want)
    mirror, out = REF.sample(g, *state)
    assert out == 0 and np.array_equal(mirror, want)
    d = sim.distributions()
    assert d["under"].tolist() == [[1, 0, 1]] and d["over"].tolist() == [[1, 0, 0]] and d["over_speed"].tolist() == [5]
    assert np.isnan(d["T_est"][0]) and np.isnan(d["mean"][0, 0]) and d["mean"][0, 1] == (-32.0 + 96.0 + 1184.0 + 32.0 * 37) / 40
    # an axisymmetric grid: a particle on the axis takes c1 = vx, c2 = vy; one on the x axis at x < 0 has c1 = -vx, c2 = -vy
    ga = VD.make_grid("axisymmetric", (1, 1), (0.0, 0.0), (p.R_oa, p.H), hist_bins=64, v_max=2048.0)
    xa, ya = x.copy(), 0.5 * x
    xa[0] = ya[0] = 0.0
    xa[1], ya[1] = -0.25 * p.R_oa, 0.0
    va = np.zeros((n, 3))
    va[0] = (-64.0, 2048.0, 0.0)        # on the axis: c1 bin 31, c2 bin 63
    va[1] = (-64.0, 2048.0, 0.0)        # c1 = 64: bin 33, c2 = -2048: bin 0
    state = (xa, ya, state[2], va[:, 0].copy(), va[:, 1].copy(), va[:, 2].copy())
    sim.set_state(*state)
    sim.enable_distributions(ga)
    sim.distributions_sample()
    tot, ns, no = sim.engine.vdf_read()
    s = VD.split(ga, tot)
    assert (ns, no) == (1, 0) and s["count"][0] == 40
    assert s["hist"][0, 0, 31] == 1 and s["hist"][0, 0, 33] == 1 and s["hist"][0, 0, 32] == 38
    assert s["hist"][0, 1, 63] == 1 and s["hist"][0, 1, 0] == 1 and s["hist"][0, 1, 32] == 38 and s["hist_speed"][0, 63] == 0
    assert s["over_speed"][0] == 2      # sqrt(64^2 + 2048^2)
    mirror, out = REF.sample(ga, *state)
    assert out == 0 and np.array_equal(tot, mirror)
    sim.close()


# ---- 5. the samplers' range is checked --------------------------------------------------------------------------------------------
def test_range_edge_is_reported_with_its_index_and_the_value_below_is_counted():
    from argon_monte_carlo_amd._lib import ArgonMCError
    from argon_monte_carlo_amd.sim import Simulation
    sim = Simulation("cube", n=1000)
    p = sim.params
    x, y, z, vx, vy, vz = IC.cube_ic(p, sim.consts, 7)
    vx, vz = vx.copy(), vz.copy()
    top = float(np.nextafter(2.0 ** 14, 0))
    vx[417], vz[600], vz[601] = 2.0 ** 14, -(2.0 ** 14), top
    sim.set_state(x, y, z, vx, vy, vz)
    sim.enable_distributions()
    sim.distributions_sample()
    with pytest.raises(ArgonMCError) as e:
        sim.engine.vdf_read()
    assert e.value.code == -4 and "particle 417 " in str(e.value)
    sim.distributions_sample()          # nothing is added while the error stands
    with pytest.raises(ArgonMCError):
        sim.engine.vdf_read()
    sim.distributions_reset()
    tot, ns, no = sim.engine.vdf_read()
    assert ns == 0 and no == 0 and not tot.any()
    # the largest magnitude in range is accepted and lands in the tails
    vx[417], vz[600] = -top, -top
    vx[601] = vy[601] = top
    sim.set_state(x, y, z, vx, vy, vz)
    sim.distributions_sample()
    ref = Totals(sim.engine.vdf_grid)
    ref.add(x, y, z, vx, vy, vz)
    s = VD.split(sim.engine.vdf_grid, ref.check(sim.engine))
    assert s["under"].sum(axis=0).tolist() == [1, 0, 1] and s["over"].sum(axis=0).tolist() == [1, 1, 1] and s["over_speed"].sum() == 3
    # NaN is reported the same way ...
    vy = vy.copy()
    vy[333] = math.nan
    sim.set_state(x, y, z, vx, vy, vz)
    sim.distributions_sample()
    with pytest.raises(ArgonMCError) as e:
        sim.engine.vdf_read()
    assert e.value.code == -4 and "particle 333 " in str(e.value)
    # ... but not on a particle outside the grid: its velocity is not examined
    half = VD.make_grid("cartesian", (1, 1, 1), (0.0, 0.0, 0.0), (0.5 * p.cube_x, p.cube_y, p.cube_z))
    out = int(np.flatnonzero(x > 0.5 * p.cube_x)[0])
    vy[333] = 0.0
    vy[out] = math.nan
    vz[out] = 2.0 ** 15
    sim.set_state(x, y, z, vx, vy, vz)
    sim.enable_distributions(half)
    sim.distributions_sample()
    tot, ns, no = sim.engine.vdf_read()
    assert ns == 1 and no == int((x > 0.5 * p.cube_x).sum()) and int(tot[0, 0]) + no == 1000
    sim.close()


# ---- 6. state errors ----------------------------------------------------------------------------------------------------------------
def test_calls_before_a_config_return_state_errors():
    from argon_monte_carlo_amd._lib import ArgonMCError
    sim = _sim("cube", 1000)
    for call in (sim.engine.lib.amc_vdf_sample, sim.engine.lib.amc_vdf_reset):
        assert call(sim.engine._ctx) == -6
    assert sim.engine.lib.amc_vdf_read(sim.engine._ctx, None, None, None) == -6
    one = np.zeros(1, dtype=np.int64)
    assert sim.engine.lib.amc_vdf_load(sim.engine._ctx, one.ctypes.data_as(sim.engine.lib.amc_vdf_load.argtypes[1]), 0, 0) == -6
    with pytest.raises(ArgonMCError) as e:
        sim.engine.vdf_read()
    assert e.value.code == -6
    sim.enable_distributions(every=1)
    sim.run(2)
    assert sim.engine.vdf_read()[1] == 2
    sim.engine.reset_outputs()          # leaves the distributions alone
    tot, ns, _ = sim.engine.vdf_read()
    assert ns == 2 and int(tot[:, 0].sum()) == 2000
    sim.disable_distributions()
    with pytest.raises(ArgonMCError) as e:
        sim.distributions_sample()
    assert e.value.code == -6 and sim.engine.vdf_grid is None
    for field, value in (("n1", 47), ("hist_bins", 257), ("hist_bins", 0), ("v_max", 0.0), ("v_max", math.inf), ("v_max", 16385.0)):
        g = VD.default_grid(sim.params)     # 8 regions x 264 columns
        setattr(g, field, value)            # past the Python helper (n1 = 47: 188 regions, 49,632 columns): the library refuses it too
        with pytest.raises(ArgonMCError) as e:
            sim.engine.vdf_config(g)
        assert e.value.code == -1, (field, value)
    g = VD.make_grid("cartesian", (93, 1, 1), (0, 0, 0), (1, 1, 1))      # 93 x 264 = 24,552 columns fit, 94 x 264 = 24,816 do not
    sim.engine.vdf_config(g)
    g.n1 = 94
    with pytest.raises(ArgonMCError) as e:
        sim.engine.vdf_config(g)
    assert e.value.code == -1
    sim.close()


# ---- 8. checkpoints ------------------------------------------------------------------------------------------------------------
def test_checkpoint_resume_gives_the_same_totals(tmp_path):
    ck = str(tmp_path / "ck.npz")
    ref_tot = SP.uninterrupted(SP.DISTRIBUTIONS, 20_000)
    a = SP.checkpointed(SP.DISTRIBUTIONS, 20_000, ck)
    a.write_distributions(str(tmp_path / "distributions.npz"))
    a.close()
    zc = np.load(ck)
    assert zc["vdf_grid"].shape == (14,) and zc["vdf_totals"].shape == (32, 264) and zc["vdf_counters"].tolist() == [2, 0]
    z = np.load(str(tmp_path / "distributions.npz"))
    assert z["totals"].shape == (32, 264) and z["pdf"].shape == (32, 3, 64) and z["pdf_speed"].shape == (32, 64) and int(z["n_samples"]) == 2
    assert z["under"].shape == z["over"].shape == z["mean"].shape == z["variance"].shape == (32, 3)
    assert z["count"].shape == z["over_speed"].shape == z["T_est"].shape == z["mean_speed"].shape == (32,)
    assert z["edges_v"].shape == z["edges_speed"].shape == (65,) and z["edges_1"].shape == (2,) and z["edges_2"].shape == (33,) and "edges_3" not in z
    assert z["shape"].tolist() == [1, 32, 1] and int(z["kind"]) == 1 and int(z["n_outside"]) == 0
    tot = SP.resumed(SP.DISTRIBUTIONS, 20_000, ck, ref_tot)
    assert int(tot[0][:, 0].sum()) == 5 * 20_000
    c = _sim("pore", 20_000)            # a checkpoint without distributions: sampling is off in the resumed run
    c.run(1)
    c.save_checkpoint(str(tmp_path / "plain.npz"))
    c.enable_distributions(every=1)
    c.load_checkpoint(str(tmp_path / "plain.npz"))
    assert c.engine.vdf_grid is None
    c.close()


# ---- 9. load and read ------------------------------------------------------------------------------------------------------------------
def test_load_read_round_trip_and_a_sample_adds_exactly():
    from argon_monte_carlo_amd.engine import Engine
    n = 40
    p, c = PR.pore_params(n=n)
    g = VD.make_grid("cartesian", (2, 1, 1), (-p.R_oa, -p.R_oa, 0.0), (p.R_oa, p.R_oa, p.H), hist_bins=8, v_max=800.0)
    k = np.arange(n)
    x = np.where(k % 2 == 0, -0.2, 0.2) * p.R_oa
    state = (x, np.zeros(n), np.full(n, 0.5 * p.H), 10.0 + 30.0 * k, -(25.0 * k), 950.0 - 50.0 * k)
    one, out = REF.sample(g, *state)
    assert out == 0 and one[:, 0].tolist() == [20, 20] and VD.split(g, one)["over"].sum() > 0 and VD.split(g, one)["under"].sum() > 0
    rng = np.random.RandomState(9)
    loaded = rng.randint(0, 1000, size=one.shape).astype(np.int64)
    big = (1 << 62) - 3
    loaded[0, 0], loaded[1, 5], loaded[1, 39], loaded[0, 20] = big, big + 2, big - 1000, big
    eng = Engine(p)
    eng.vdf_config(g)
    eng.vdf_load(loaded, 9, 2)
    tot, ns, no = eng.vdf_read()
    assert (ns, no) == (9, 2) and np.array_equal(tot, loaded)
    eng.upload(*state)
    eng.vdf_sample()
    tot, ns, no = eng.vdf_read()
    assert (ns, no) == (10, 2)
    assert np.array_equal(tot, loaded + one), np.argwhere(tot != loaded + one)[:5]
    assert int(tot[0, 0]) == big + 20
    with pytest.raises(ValueError):
        eng.vdf_load(loaded[:, :-1], 0, 0)
    eng.close()


# ---- 10. energised pore: host-RNG and device-RNG steps, and the host-free run ---------------------------------------------------
@pytest.mark.parametrize("device_rng", [False, True])
def test_energised_pore_totals_equal_reference(device_rng, tmp_path):
    sim, ref, tot = SP.energised_totals(SP.DISTRIBUTIONS, device_rng, every=2)
    assert ref.n_samples == 2 and int(tot[:, 0].sum()) + ref.n_outside == 40_000
    d = sim.distributions()
    assert np.isfinite(d["pdf_speed"][d["count"] >= 1]).all()
    read, state = sim.engine.vdf_read(), sim.engine.download()
    ck = str(tmp_path / "ck.npz")
    sim.save_checkpoint(ck)             # the energised class extends the base class's checkpoint: the distributions travel with it
    sim.close()
    z = np.load(ck)
    assert np.array_equal(z["vdf_totals"], tot) and z["vdf_counters"].tolist() == [2, ref.n_outside]
    if device_rng:                      # the host-free run takes the same samples as four single steps
        SP.host_free_run(SP.DISTRIBUTIONS, read, state, every=2)


# ---- 12. physics on a Maxwell start ---------------------------------------------------------------------------------------------
def test_maxwell_start_gives_maxwellian_histograms_and_its_temperature():
    """Cube, n = 100,000, seed 3, one region, one sample.  The device's counts are the mirror's, so Pearson's chi-square against the
    bin-integrated Maxwell distribution is the host test's: 20.4, 34.3, 25.7 over 30 bins (bound 30 + 6 sqrt(60) = 76.5) and 26.4
    over 36 bins for the speed (bound 86.9).  T_est puts every count at its bin's midpoint: that adds w^2 / 12 = 64^2 / 12 to each
    component's variance (341 of 62,400 m^2/s^2: 1.6 K), so T_est must lie within 64^2 m / (12 k_B) plus six standard errors of
    m a_shape^2 / k_B; the standard error of the mean of (C1^2 + C2^2 + C3^2) / 3 comes from the downloaded velocities."""
    n = 100_000
    sim = _sim("cube", n, seed=3)
    p = sim.params
    g = VD.make_grid("cartesian", (1, 1, 1), (0.0, 0.0, 0.0), (p.cube_x, p.cube_y, p.cube_z))
    sim.enable_distributions(g)
    sim.distributions_sample()
    st = sim.engine.download()
    ref = Totals(g)
    ref.add_state(st)
    tot = ref.check(sim.engine)
    d = sim.distributions()
    m, k_b = float(p.argon_mass), VD.boltzmann_constant(p)
    assert d["n_outside"] == 0 and d["count"].tolist() == [n] and not d["under"].any() and not d["over"].any() and not d["over_speed"].any()
    res = REF.maxwell_chi_squares(g, tot, sim.consts, m, k_b)
    print("chi-square, cells:", res)
    assert [k for _, k in res] == [30, 30, 30, 36]
    for chi2, k in res:
        assert chi2 < k + 6.0 * math.sqrt(2.0 * k), (chi2, k)
    c = np.stack([st["vx"], st["vy"], st["vz"]])
    C = c - c.mean(axis=1, keepdims=True)
    se = float(np.std((C * C).sum(axis=0) / 3.0)) / math.sqrt(n)
    T0 = m * float(sim.consts["a_shape"]) ** 2 / k_b
    bound = 64.0 ** 2 * m / (12.0 * k_b) + 6.0 * m / k_b * se
    print("T_est", d["T_est"][0], "T0", T0, "bound", bound)
    assert abs(d["T_est"][0] - T0) < bound
    sim.close()
