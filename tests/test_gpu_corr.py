"""GPU (-m gpu): sampled correlations (include/argonmc.h "sampled correlations").  The device's integer totals must equal the
Python-int reference (tests/corr_ref.py) on the downloaded states bit for bit, whatever the launch configuration or the way the
steps were driven, and sampling must change nothing else.  What the correlations share with the other streaming samplers — two
ranks, odd index ranges, sampling changes nothing else — is in tests/test_gpu_sampler_protocol.py, and the body of run(k)
against k timesteps in tests/sampler_protocol.py."""
import numpy as np
import pytest

from argon_monte_carlo_amd import correlations as CO
from argon_monte_carlo_amd import fields as FL
from argon_monte_carlo_amd import ic as IC
from argon_monte_carlo_amd import params as PR
from tests import corr_ref as REF
from tests import sampler_protocol as SP
from tests.sampler_protocol import KEYS, N
from tests.sampler_protocol import CorrMirror as Window
from tests.sampler_protocol import make_sim as _sim

pytestmark = pytest.mark.gpu

_grid = SP.CORRELATIONS.grids


# ---- 1. the totals equal the reference on the downloaded states ----------------------------------------------------------
@pytest.mark.parametrize("kind,which,n,blocks", [("cube", "default", N, None), ("cube", "444", N, None), ("pore", "default", N, None),
                                                 ("pore", "one", N, None), ("pore", "default", 100_003, "256")])
def test_totals_equal_reference_after_timesteps(kind, which, n, blocks, monkeypatch):
    if blocks is not None:              # the full persistent grid: one workgroup per CU of the largest part
        monkeypatch.setenv("AMC_CORR_BLOCKS", blocks)
    sim = _sim(kind, n)
    sim.enable_correlations(_grid(kind, sim.params, which, 3))
    win = Window(sim.engine.corr_grid)
    sim.correlations_sample()           # straight after the upload: the first origin
    win.add_state(sim.engine.download())
    for _ in range(7):                  # lags 1, 2, 3 + origin, 1, 2, 3 + origin, 1: two turnovers, the end mid-window
        sim.timestep()
        sim.correlations_sample()       # the cube's sweep results are still deferred here: read through the slot arrays
        win.add_state(sim.engine.download())
    tot = CO.words_to_ints(win.check(sim.engine))
    assert win.counters()[0] == 3 and win.counters()[3] == 2
    assert sum(int(v) for v in tot[:, 0, 0]) + win.n_outside == 3 * n           # counts plus outside, per origin
    assert any(int(v) != 0 for v in tot[:, 3, 1]) and any(int(v) != 0 for v in tot[:, 1, 4])
    sim.close()


# ---- 2. run(k) equals k timesteps, for any number of workgroups and in an overlapped run ----------------------------------
@pytest.mark.parametrize("kind,overlap,blocks", [("cube", None, None), ("pore", None, None), ("cube", "1", None), ("pore", "1", None),
                                                 ("cube", None, "1"), ("pore", None, "1"), ("cube", None, "7"), ("pore", None, "7")])
def test_run_equals_timesteps_and_reference(kind, overlap, blocks, monkeypatch):
    SP.check_run(SP.CORRELATIONS, monkeypatch, kind, None, overlap, blocks)


# ---- 4. together with the fields: one "any sampler due" predicate ------------------------------------------------------------
def test_fields_and_correlations_in_one_run_equal_each_alone():
    got = {}
    for which in ("both", "fields", "corr"):
        sim = _sim("pore", N, seed=6)
        if which != "corr":
            sim.enable_fields(every=3)
        if which != "fields":
            sim.enable_correlations(every=2, n_lags=2)
        sim.run(12)
        got[which] = (sim.engine.fields_read() if which != "corr" else None, sim.engine.corr_read() if which != "fields" else None,
                      sim.engine.download())
        sim.close()
    (f_tot, f_ns, f_no), (f1_tot, f1_ns, f1_no) = got["both"][0], got["fields"][0]
    assert f_ns == f1_ns == 4 and f_no == f1_no and np.array_equal(f_tot, f1_tot)
    (c_tot, c_cnt), (c1_tot, c1_cnt) = got["both"][1], got["corr"][1]
    assert c_cnt == c1_cnt and c_cnt[:2] == (3, 6) and np.array_equal(c_tot, c1_tot) and c_tot.any()
    for k in KEYS:
        assert np.array_equal(got["both"][2][k], got["fields"][2][k]) and np.array_equal(got["both"][2][k], got["corr"][2][k]), k


# ---- 5. lag 0 against the fields ----------------------------------------------------------------------------------------------
def test_lag_zero_products_equal_the_fields_second_moments():
    sim = _sim("cube", N, seed=3)
    p = sim.params
    sim.enable_fields(FL.make_grid("cartesian", (1, 1, 1), (0, 0, 0), (p.cube_x, p.cube_y, p.cube_z)))
    sim.enable_correlations(_grid("cube", p, "one", 2))
    sim.timestep()
    sim.fields_sample()
    sim.correlations_sample()
    f = FL.words_to_ints(sim.engine.fields_read()[0])
    tot, counters = sim.engine.corr_read()
    c = CO.words_to_ints(tot)
    assert counters == (1, 1, 0, 1)
    assert int(c[0, 0, 0]) == int(f[0, 0]) == N
    for k in range(3):
        assert int(c[0, 0, 4 + k]) == int(f[0, 4 + k]) > 0 and int(c[0, 0, 1 + k]) == 0
    assert not tot[:, 1:].any()
    sim.close()


# ---- 6. zero velocities ------------------------------------------------------------------------------------------------------
def test_zero_velocities_give_zero_sums_and_full_counts():
    from argon_monte_carlo_amd.sim import Simulation
    sim = Simulation("cube", n=N)
    x, y, z, vx, vy, vz = IC.cube_ic(sim.params, sim.consts, 2)
    zero = np.zeros(N)
    sim.set_state(x, y, z, zero, zero, zero)
    sim.enable_correlations(n_lags=3)
    for _ in range(3):
        sim.correlations_sample()
    c = CO.words_to_ints(sim.engine.corr_read()[0])
    assert [int(c[0, l, 0]) for l in range(4)] == [N, N, N, 0]
    sim.correlations_sample()           # lag 3, and the next origin
    tot, counters = sim.engine.corr_read()
    c = CO.words_to_ints(tot)
    assert counters == (2, 4, 0, 1) and [int(c[0, l, 0]) for l in range(4)] == [2 * N, N, N, N]
    assert not tot[:, :, 1:].any()      # every m_k and c_k, at every lag
    sim.close()


# ---- 7. the quantisers' range is checked, not wrapped ----------------------------------------------------------------------
def test_velocity_out_of_range_is_reported_not_summed():
    from argon_monte_carlo_amd._lib import ArgonMCError
    from argon_monte_carlo_amd.sim import Simulation
    sim = Simulation("cube", n=1000)
    x, y, z, vx, vy, vz = IC.cube_ic(sim.params, sim.consts, 7)
    vx = vx.copy()
    vx[417] = 2.0 ** 14
    vx[600] = -(2.0 ** 14)
    sim.set_state(x, y, z, vx, vy, vz)
    sim.enable_correlations()
    sim.correlations_sample()
    with pytest.raises(ArgonMCError) as e:
        sim.engine.corr_read()
    assert e.value.code == -4 and "particle 417 " in str(e.value)
    sim.correlations_reset()
    tot, counters = sim.engine.corr_read()
    assert counters == (0, 0, 0, 0) and not tot.any()
    sim.close()


def test_displacement_out_of_range_is_reported_not_summed():
    from argon_monte_carlo_amd._lib import ArgonMCError
    from argon_monte_carlo_amd.sim import Simulation
    sim = Simulation("cube", n=1000)
    x, y, z, vx, vy, vz = IC.cube_ic(sim.params, sim.consts, 7)
    sim.set_state(x, y, z, vx, vy, vz)
    sim.enable_correlations()
    sim.correlations_sample()           # the origin
    tot0, counters0 = sim.engine.corr_read()
    assert counters0 == (1, 1, 0, 1)
    moved = np.array(x, dtype=np.float64)
    moved[5] = x[5] + 2.0 ** -18
    if moved[5] - x[5] < 2.0 ** -18:    # (the sum was rounded down: the next double is 2^-18 away or more)
        moved[5] = np.nextafter(moved[5], np.inf)
    assert moved[5] - x[5] >= 2.0 ** -18
    sim.engine.upload(x=moved)          # an upload restarts no window
    sim.correlations_sample()
    with pytest.raises(ArgonMCError) as e:
        sim.engine.corr_read()
    assert e.value.code == -4 and "particle 5 " in str(e.value)
    sim.correlations_reset()
    tot, counters = sim.engine.corr_read()
    assert counters == (0, 0, 0, 0) and not tot.any()
    sim.close()


# ---- 8. checkpoints ------------------------------------------------------------------------------------------------------------
def test_checkpoint_resume_mid_window_gives_the_same_totals(tmp_path):
    from argon_monte_carlo_amd.sim import Simulation
    ref = _sim("pore", N, seed=4)
    ref.enable_correlations(every=3, n_lags=2)
    ref.run(7)
    ref.run(8)
    ref_tot, ref_cnt = ref.engine.corr_read()
    ref.close()
    a = _sim("pore", N, seed=4)
    a.enable_correlations(every=3, n_lags=2)
    a.run(7)                            # samples at steps 3 (origin) and 6 (lag 1): saved mid-window
    mid = a.engine.corr_read()[1]
    assert mid[:2] == (1, 2) and mid[3] == 2
    ck = str(tmp_path / "ck.npz")
    a.save_checkpoint(ck)
    a.close()
    b = Simulation("pore", n=N)
    b.load_checkpoint(ck)               # restores the grid, totals, counters, window position and origin arrays
    b.run(8)                            # steps 9 (lag 2 + origin), 12, 15 (lag 2 + origin)
    tot, cnt = b.engine.corr_read()
    assert cnt == ref_cnt and cnt[:2] == (3, 5) and cnt[3] == 1
    assert np.array_equal(tot, ref_tot) and tot[:, 2].any()
    b.close()


def test_checkpoint_without_correlations_loads_with_sampling_off(tmp_path):
    from argon_monte_carlo_amd._lib import ArgonMCError
    from argon_monte_carlo_amd.sim import Simulation
    a = _sim("cube", 1000)
    a.run(2)
    ck = str(tmp_path / "ck.npz")
    a.save_checkpoint(ck)
    a.close()
    b = Simulation("cube", n=1000)
    b.enable_correlations(every=1)
    b.load_checkpoint(ck)
    assert b.engine.corr_grid is None
    with pytest.raises(ArgonMCError) as e:
        b.correlations_sample()
    assert e.value.code == -6
    b.close()


# ---- 9. energised pore: host-RNG and device-RNG steps --------------------------------------------------------------------------
@pytest.mark.parametrize("device_rng", [False, True])
def test_energised_pore_totals_equal_reference(device_rng):
    sim, win, tot = SP.energised_totals(SP.CORRELATIONS, device_rng, every=1, n_lags=2)     # origin, lag 1, lag 2 + origin, lag 1
    assert win.counters()[:2] == (2, 4) and tot[:, 1:, 1:4].any()
    f = sim.correlations()
    assert np.isfinite(f["msd"][f["count"] > 0]).all()
    read, state = sim.engine.corr_read(), sim.engine.download()
    sim.close()
    if device_rng:                      # the host-free run takes the same samples as four single steps
        SP.host_free_run(SP.CORRELATIONS, read, state, every=1, n_lags=2)


# ---- 11. physics, derivable ------------------------------------------------------------------------------------------------------
def test_maxwell_initial_condition_reads_back_the_velocity_variance():
    n = 100_000
    sim = _sim("cube", n, seed=3)
    sim.enable_correlations(_grid("cube", sim.params, "one", 4))
    sim.correlations_sample()
    f = sim.correlations()
    a2 = float(sim.consts["a_shape"]) ** 2
    sigma = a2 * np.sqrt(2.0 / n)
    assert f["count"][0, 0] == n and f["n_outside"] == 0
    for k in range(3):
        assert abs(f["vacf"][0, 0, k] - a2) < 4 * sigma, (k, f["vacf"][0, 0, k], a2, sigma)
        assert f["msd"][0, 0, k] == 0.0
    sim.close()


# ---- 13. the carry-add through the correlations' loads ------------------------------------------------------------------------------
def test_corr_load_carry_and_borrow():
    """128-bit totals: loaded low words of 2^64 - 1 carry into the high word under a positive sum, low words of 0 borrow from it
    under a negative one (velocity products against an origin of the opposite sign); the result equals the exact Python-int sum.
    Three samples with n_lags = 2: every mode of the accumulate kernel feeds the carry-add."""
    from argon_monte_carlo_amd.engine import Engine
    n = 40
    k = np.arange(n)
    g = CO.make_grid("cartesian", (2, 1, 1), (-1.0e-7, -1.0e-7, 0.0), (1.0e-7, 1.0e-7, 1.0e-6), n_lags=2)
    x, y, z = np.where(k % 2 == 0, -5.0e-8, 5.0e-8), np.zeros(n), np.full(n, 5.0e-7)
    vx, vy, vz = 300.0 + k, 120.5 + 0.25 * k, 77.0 + k
    states = [(x, y, z, vx, vy, vz), (x + 1e-10, y - 2e-10, z + 3e-10, -vx, -vy, -vz), (x + 2e-10, y - 4e-10, z + 6e-10, -vx, -vy, -vz)]
    win = REF.Window(g)
    for st in states:
        win.add(st)
    sums = win.totals
    assert win.n_outside == 0 and all(int(v) < 0 for v in sums[:, 1:, 4:].ravel()) and all(int(v) > 0 for v in sums[:, 1:, :4].ravel())
    loaded = np.empty(sums.shape, dtype=object)
    for idx in np.ndindex(sums.shape):
        loaded[idx] = (1 << 64) - 1 if sums[idx] > 0 else 0
    loaded[0, 0, 0] = (5 << 64) - 1                                  # high word already non-zero
    lw, ew = CO.ints_to_words(loaded), CO.ints_to_words(loaded + sums)
    carry, borrow = ew[..., 1] > lw[..., 1], ew[..., 1] < lw[..., 1]
    assert carry.sum() == (sums > 0).sum() and borrow.sum() == (sums < 0).sum() == 2 * 2 * 3
    p, _ = PR.pore_params(n=n)
    eng = Engine(p)
    eng.corr_config(g)
    eng.corr_load(lw, (5, 9, 2, 0))
    for st in states:
        eng.upload(*st)
        eng.corr_sample()
    tot, counters = eng.corr_read()
    assert counters == (7, 12, 2, 1)
    assert np.array_equal(tot, ew), np.argwhere(tot != ew)[:5]
    eng.close()
