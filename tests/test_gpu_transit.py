"""GPU (-m gpu): sampled transits (include/argonmc_transit.h).  The device's integer totals must equal the mirror
(tests/transit_ref.py) on the downloaded states bit for bit, whatever the launch configuration or the way the steps were driven,
and sampling must change nothing else.  What the transits share with the other streaming samplers — two ranks, odd index ranges,
sampling changes nothing else — is in tests/test_gpu_sampler_protocol.py, and the body of run(k) against k timesteps in
tests/sampler_protocol.py."""
import math
import os

import numpy as np
import pytest

from argon_monte_carlo_amd import params as PR
from argon_monte_carlo_amd import transits as TR
from argon_monte_carlo_amd.totals import ints_to_words, words_to_ints
from tests import sampler_protocol as SP
from tests import transit_ref as REF
from tests.sampler_protocol import KEYS
from tests.sampler_protocol import TransitMirror as Mirror
from tests.sampler_protocol import make_sim as _sim
from tests.sampler_protocol import thin_zones as _thin_zones
from tests.sampler_protocol import transit_classes as _classes
from tests.sampler_protocol import transit_zones as _zones
from tests.sampler_states import ODD_N, drifting_states

pytestmark = pytest.mark.gpu

COL = TR.class_column


# ---- 1. the totals equal the mirror on the downloaded states ------------------------------------------------------------------
@pytest.mark.parametrize("kind,n,steps,every,offset", [("cube", 1_000, 60, 1, 0), ("cube", 1_000, 60, 3, 1), ("pore", ODD_N, 80, 1, 0)])
def test_totals_equal_mirror_after_timesteps(kind, n, steps, every, offset):
    sim = _sim(kind, n)
    zones = _zones(kind, sim.params)
    sim.engine.transit_config(TR.make_grid(zones, every=every, step_offset=offset))
    m = Mirror(zones, n)
    for s in range(1, steps + 1):
        sim.timestep()
        st = sim.engine.download()
        if (s + offset) % every == 0:
            m.add_state(st)
    t = m.check(sim.engine)
    assert m.n_samples == (steps + offset) // every
    hit = [any(_classes(t, k)[c] > 0 for k in range(len(zones))) for c in range(6)]
    print("exits per zone and class:", [_classes(t, k) for k in range(len(zones))], "skipped", [int(t[k, 3]) for k in range(len(zones))])
    # nothing compares zeros only: whole residences complete (the pore's few atoms near its thin zones give a handful) ...
    assert sum(hit) >= 2 and all(int(t[k, 0:3].sum()) > 0 for k in range(len(zones))), hit
    if kind == "cube":                  # ... and the thirds give every class (entry side, exit side) in some zone:
        assert all(hit), hit            # a wall is behind the outer thirds; the middle one transmits
        assert _classes(t, 0)[2] == 0 and _classes(t, 2)[1] == 0 and _classes(t, 1)[1] > 0 and _classes(t, 1)[2] > 0
    d = sim.transits()
    assert d["n_samples"] == m.n_samples and d["inside_now"].tolist() == m.inside_counts[-1]
    assert d["interval"] == every * sim.dt and (kind != "cube" or np.isfinite(d["transmission"][1]).all())
    sim.close()


# ---- 2. run(k) equals k timesteps equals the mirror, for any number of workgroups, overlapped, beside another sampler ------------
@pytest.mark.parametrize("kind,overlap,blocks,mfp", [
    ("cube", None, None, False), ("pore", None, None, False), ("cube", None, "1", False), ("pore", None, "1", False),
    ("cube", None, "3", False), ("pore", None, "3", False), ("cube", "1", None, False), ("pore", "1", None, False),
    ("cube", None, None, True), ("pore", None, None, True)])
def test_run_equals_timesteps_and_mirror(kind, overlap, blocks, mfp, monkeypatch):
    SP.check_run(SP.TRANSITS, monkeypatch, kind, None, overlap, blocks, mfp)


# ---- 4. crafted edges -----------------------------------------------------------------------------------------------------------------
def test_crafted_edges_land_in_the_documented_columns():
    """Zone A = [lo, hi) = [0.25, 0.5) of x (in units of the cube's edge) and B = [0.3, 0.4) nested in it; eleven particles are
    moved by upload between eleven samples taken by hand.  Zone A's expected columns are written out by hand."""
    from argon_monte_carlo_amd.sim import Simulation
    n = 12
    sim = Simulation("cube", n=n)
    L = float(sim.params.cube_x)
    lo, hi = 0.25 * L, 0.5 * L
    zones = [(0, lo, hi), (0, 0.3 * L, 0.4 * L)]
    below, inside, above = 0.1 * L, 0.27 * L, 0.7 * L          # (inside A, below B)
    frames = 11
    X = np.full((frames, n), below)
    X[:, 0] = lo                                                # u == lo is inside: there at the first sample, entry side 2, never leaves
    X[:, 1] = hi                                                # u == hi is above
    X[:, 2] = np.nextafter(lo, -math.inf)                       # below
    X[1:, 3] = above                                            # below -> above in one sample: skipped, nothing else
    X[1, 4], X[2:, 4] = inside, above                           # entry and exit in consecutive samples: tau = 1, column 0, class (below, above)
    for p, tau in zip(range(5, 10), (2, 3, 4, 7, 8)):           # from above, out below: columns 1, 1, 2, 2, 3
        X[0, p] = above
        X[1:1 + tau, p] = inside
    X[1:3, 10], X[3:6, 10], X[6:, 10] = 0.35 * L, 0.45 * L, above      # inside both; leaves B (upwards) after 2 samples, A after 5
    X[0, 11], X[1:, 11] = 0.35 * L, below                       # inside both when first seen, out below after one sample
    half = np.full(n, 0.5 * L)
    zero = np.zeros(n)
    sim.enable_transits(TR.make_grid(zones), every=0)
    m = Mirror(zones, n)
    for f in range(frames):
        sim.set_state(X[f].copy(), half, half, zero, zero, zero)
        sim.transits_sample()
        m.sample(X[f], half, half)
    t = m.check(sim.engine)
    a = np.zeros(263, dtype=object)
    a[0], a[1], a[2], a[3] = 2, 5, 2, 1                         # entries from below (4, 10), above (5 .. 9), already inside (0, 11); skipped (3)
    a[4] = frames + 1 + (2 + 3 + 4 + 7 + 8) + 5 + 1             # inside_sum: particle 0 always, 4 once, the five residences, 10 five times, 11 once
    a[COL(0, 1)], a[COL(0, 1, 1)], a[COL(0, 1, 2)] = 2, 1 + 5, 1 + 25
    a[COL(0, 1, 3 + 0)], a[COL(0, 1, 3 + 2)] = 1, 1             # tau 1 -> column 0, tau 5 -> column 2
    a[COL(1, 0)], a[COL(1, 0, 1)], a[COL(1, 0, 2)] = 5, 24, 4 + 9 + 16 + 49 + 64
    a[COL(1, 0, 3 + 1)], a[COL(1, 0, 3 + 2)], a[COL(1, 0, 3 + 3)] = 2, 2, 1
    a[COL(2, 0)], a[COL(2, 0, 1)], a[COL(2, 0, 2)], a[COL(2, 0, 3)] = 1, 1, 1, 1
    assert np.array_equal(t[0], a), np.flatnonzero(t[0] != a)
    # zone B: particle 10 leaves it at another sample than zone A (tau 2, upwards); the jumps over it are skipped crossings
    assert int(t[1, COL(0, 1)]) == 1 and int(t[1, COL(0, 1, 1)]) == 2 and int(t[1, COL(0, 1, 3 + 1)]) == 1
    assert int(t[1, COL(2, 0)]) == 1 and int(t[1, 0]) == 1 and int(t[1, 1]) == 0 and int(t[1, 2]) == 1
    assert int(t[1, 3]) == 1 + 1 + 5                            # 3 and 4 upwards, 5 .. 9 downwards (their stay in A is below B)
    state, entry = sim.engine.transit_state()
    assert state[0] == (2 | 2 << 2) | 1 << 4 and state[1] == 3 | 3 << 4 and state[2] == 1 | 1 << 4 and entry[0, 0] == 0
    d = sim.transits()
    assert d["inside_now"].tolist() == [1, 0] and d["transmission"][0].tolist() == [1.0, 1.0]
    sim.close()


# ---- 5. the limits, through transit_load ----------------------------------------------------------------------------------------------
def _tiny():
    from argon_monte_carlo_amd.sim import Simulation
    n = 10
    sim = Simulation("cube", n=n)
    L = float(sim.params.cube_x)
    zones = [(1, 0.25 * L, 0.5 * L)]
    sim.enable_transits(TR.make_grid(zones), every=0)
    return sim, n, L, zones


def _set_y(sim, n, L, y):
    half = np.full(n, 0.5 * L)
    sim.set_state(half, np.asarray(y, dtype=np.float64), half, np.zeros(n), np.zeros(n), np.zeros(n))
    return half, np.asarray(y, dtype=np.float64), half


def test_long_residences_are_exact_and_the_sample_limit_stops_the_sampler():
    from argon_monte_carlo_amd._lib import ArgonMCError
    sim, n, L, zones = _tiny()
    m = Mirror(zones, n)
    inside, below, above = 0.3 * L, 0.1 * L, 0.9 * L
    # particles 3 and 6 are inside, entered from below at sample 3 and from above at sample 0; everybody else below
    state = np.full(n, 1, dtype=np.uint32)
    state[3], state[6] = 2 | 0 << 2, 2 | 1 << 2
    entry = np.zeros((1, n), dtype=np.uint32)
    entry[0, 3] = 3
    t0 = np.zeros((1, 263), dtype=object)
    t0[0, 0], t0[0, 1], t0[0, 4] = 1, 1, 2 ** 70 + 12345         # (a 128-bit total survives the round trip)
    ns = 2 ** 31 + 5
    sim.engine.transit_load(ints_to_words(t0), ns, state, entry)
    m.load(ints_to_words(t0), ns, state, entry)
    tot, got = sim.engine.transit_read()
    assert got == ns and np.array_equal(tot, ints_to_words(t0))
    s2, e2 = sim.engine.transit_state()
    assert np.array_equal(s2, state) and np.array_equal(e2, entry)
    y = np.full(n, below)
    y[3], y[6] = above, inside
    m.sample(*_set_y(sim, n, L, y))
    sim.transits_sample()
    t = m.check(sim.engine)
    tau = 2 ** 31 + 2
    c = COL(0, 1)
    assert [int(v) for v in t[0, c:c + 3]] == [1, tau, tau * tau] and int(t[0, c + 3 + 31]) == 1 and tau * tau > 2 ** 62
    assert int(t[0, 4]) == 2 ** 70 + 12345 + 1
    # the largest tau: entry index 0, sample index 2^32 - 2
    tot, _ = sim.engine.transit_read()
    state, entry = sim.engine.transit_state()
    ns = 2 ** 32 - 2
    sim.engine.transit_load(tot, ns, state, entry)
    m.load(tot, ns, state, entry)
    y[6] = below
    m.sample(*_set_y(sim, n, L, y))
    sim.transits_sample()
    t = m.check(sim.engine)
    tau = 2 ** 32 - 2
    c = COL(1, 0)
    assert [int(v) for v in t[0, c:c + 3]] == [1, tau, tau * tau] and int(t[0, c + 3 + 31]) == 1 and m.n_samples == 2 ** 32 - 1
    # the sample that would be number 2^32 adds nothing and moves nobody, nor does a later one; the read says so until a reset
    before_state = sim.engine.transit_state()[0]
    y[0] = inside
    for _ in range(2):
        _set_y(sim, n, L, y)
        sim.transits_sample()
        with pytest.raises(ArgonMCError) as e:
            sim.engine.transit_read()
        assert e.value.code == -4 and "2^32 - 1" in str(e.value) and "particle" not in str(e.value)
    assert np.array_equal(sim.engine.transit_state()[0], before_state)
    sim.engine.transit_load(tot, 5, state, entry)               # a load clears it ...
    assert sim.engine.transit_read()[1] == 5
    sim.engine.transit_load(tot, 2 ** 32 - 1, state, entry)
    sim.transits_sample()
    with pytest.raises(ArgonMCError):
        sim.engine.transit_read()
    sim.transits_reset()                                        # ... and so does a reset
    tot, ns = sim.engine.transit_read()
    assert ns == 0 and not tot.any() and not sim.engine.transit_state()[0].any()
    # what a sample cannot leave is refused: an entry side outside the zone, side 3, a zone that is not configured, too many samples
    for word in (1 | 1 << 2, 2 | 3 << 2, 1 << 4):
        bad = np.full(n, 1, dtype=np.uint32)
        bad[4] = word
        with pytest.raises(ArgonMCError) as e:
            sim.engine.transit_load(tot, 0, bad, entry)
        assert e.value.code == -1 and "particle 4" in str(e.value)
    with pytest.raises(ArgonMCError) as e:
        sim.engine.transit_load(tot, 2 ** 32, state, entry)
    assert e.value.code == -1
    sim.close()


def test_nan_is_reported_with_its_index_and_the_sample_before_it_counted():
    from argon_monte_carlo_amd._lib import ArgonMCError
    sim, n, L, zones = _tiny()
    m = Mirror(zones, n)
    y = np.linspace(0.05, 0.95, n) * L
    half = np.full(n, 0.5 * L)
    nan = np.full(n, math.nan)
    sim.set_state(nan, y, nan, np.zeros(n), np.zeros(n), np.zeros(n))      # (axes no zone looks at are not examined)
    sim.transits_sample()
    m.sample(nan, y, nan)
    t = m.check(sim.engine)
    assert int(t[0, 2]) == int(((y >= 0.25 * L) & (y < 0.5 * L)).sum()) > 0
    y2 = y.copy()
    y2[7] = y2[9] = math.nan
    y2[2] = 0.3 * L                     # would be an entry: the sample adds nothing
    sim.set_state(half, y2, half, np.zeros(n), np.zeros(n), np.zeros(n))
    sim.transits_sample()
    with pytest.raises(ArgonMCError) as e:
        sim.engine.transit_read()
    assert e.value.code == -4 and "particle 7 " in str(e.value)
    sim.set_state(half, y, half, np.zeros(n), np.zeros(n), np.zeros(n))
    sim.transits_sample()               # nothing is added while the error stands
    with pytest.raises(ArgonMCError):
        sim.engine.transit_read()
    tot = np.zeros(TR.totals_shape(sim.engine.transit_grid), dtype=np.int64)
    assert sim.engine.lib.amc_transit_read(sim.engine._ctx, tot.ctypes.data_as(sim.engine.lib.amc_transit_read.argtypes[1]), None) == -4
    assert np.array_equal(tot, m.words())          # the totals are those of the sample before the NaN
    sim.transits_reset()
    tot, ns = sim.engine.transit_read()
    assert ns == 0 and not tot.any()
    sim.close()


# ---- 6. behaviour around the sampler ---------------------------------------------------------------------------------------------
def test_calls_before_a_config_return_state_errors():
    from argon_monte_carlo_amd._lib import ArgonMCError
    sim = _sim("cube", 1000)
    lib, ctx = sim.engine.lib, sim.engine._ctx
    for call in (lib.amc_transit_sample, lib.amc_transit_reset):
        assert call(ctx) == -6
    assert lib.amc_transit_read(ctx, None, None) == -6 and lib.amc_transit_state(ctx, None, None) == -6
    one = np.zeros(1, dtype=np.int64)
    assert lib.amc_transit_load(ctx, one.ctypes.data_as(lib.amc_transit_load.argtypes[1]), 0, None, None) == -6
    with pytest.raises(ArgonMCError) as e:
        sim.engine.transit_read()
    assert e.value.code == -6
    sim.enable_transits()
    sim.run(2)
    assert sim.engine.transit_read()[1] == 2
    sim.engine.reset_outputs()          # leaves the transits alone
    tot, ns = sim.engine.transit_read()
    assert ns == 2 and int(words_to_ints(tot)[:, 4].sum()) == 2000       # the thirds hold everybody, twice
    sim.engine.transit_config(sim.engine.transit_grid)                    # a (new) grid starts over
    tot, ns = sim.engine.transit_read()
    assert ns == 0 and not tot.any() and not sim.engine.transit_state()[0].any()
    sim.disable_transits()
    with pytest.raises(ArgonMCError) as e:
        sim.transits_sample()
    assert e.value.code == -6 and sim.engine.transit_grid is None
    for field, value in (("n_zones", 0), ("n_zones", 9), ("every", -1), ("step_offset", -1), ("struct_size", 192)):
        g = TR.default_grid(sim.params)
        setattr(g, field, value)        # past the Python helper: the library refuses it too
        with pytest.raises(ArgonMCError) as e:
            sim.engine.transit_config(g)
        assert e.value.code == -1, (field, value)
    for change in (lambda g: g.axis.__setitem__(1, 3), lambda g: g.lo.__setitem__(0, g.hi[0]), lambda g: g.hi.__setitem__(2, math.inf),
                   lambda g: g.lo.__setitem__(1, math.nan), lambda g: g.reserved.__setitem__(1, 1), lambda g: g.hi.__setitem__(5, 1.0)):
        g = TR.default_grid(sim.params)
        change(g)
        with pytest.raises(ArgonMCError) as e:
            sim.engine.transit_config(g)
        assert e.value.code == -1
    sim.close()


def test_checkpoint_mid_residence_resumes_to_the_same_totals(tmp_path):
    from argon_monte_carlo_amd.sim import Simulation
    n = 20_000
    ref = _sim("pore", n, seed=4)
    grid = TR.make_grid(_thin_zones(ref.params))
    ref.enable_transits(grid, every=2)
    ref.run(13)
    ref.run(16)
    ref_tot, ref_ns = ref.engine.transit_read()
    ref_state = ref.engine.transit_state()[0]
    ref.close()
    a = _sim("pore", n, seed=4)
    a.enable_transits(grid, every=2)
    a.run(13)
    ck = str(tmp_path / "ck.npz")
    a.save_checkpoint(ck)
    a.write_transits(str(tmp_path / "transits.npz"))
    state_a = a.engine.transit_state()[0]
    a.close()
    assert int((((state_a >> np.uint32(4)) & np.uint32(3)) == 2).sum()) > 0      # residences are under way at the checkpoint
    zc = np.load(ck)
    assert zc["transit_grid"].shape == (27,) and zc["transit_totals"].shape == (3, 263, 2) and zc["transit_counters"].tolist() == [6]
    assert zc["transit_state"].shape == (n,) and zc["transit_state"].dtype == np.uint32 and zc["transit_entry"].shape == (3, n)
    z = np.load(str(tmp_path / "transits.npz"))
    assert z["totals"].shape == (3, 263, 2) and z["transmission"].shape == (3, 2) and z["residence_mean"].shape == (3, 3, 2)
    assert z["hist"].shape == (3, 3, 2, 40) and z["hist_edges_s"].shape == (41,) and int(z["n_samples"]) == 6 and z["zones"].shape == (3, 3)
    b = Simulation("pore", n=n)
    b.load_checkpoint(ck)               # restores the zones, the totals, the per-particle arrays and the cadence (steps 14, 16 .. 28 to come)
    b.run(16)
    tot, ns = b.engine.transit_read()
    assert ns == ref_ns == 14 and np.array_equal(tot, ref_tot) and np.array_equal(b.engine.transit_state()[0], ref_state)
    assert sum(sum(_classes(words_to_ints(tot), k)) for k in range(3)) > 0
    b.close()
    c = _sim("pore", n)                 # a checkpoint without transits: sampling is off in the resumed run
    c.run(1)
    c.save_checkpoint(str(tmp_path / "plain.npz"))
    c.enable_transits()
    c.load_checkpoint(str(tmp_path / "plain.npz"))
    assert c.engine.transit_grid is None
    c.close()


def test_load_read_round_trip_and_a_sample_adds_exactly():
    from argon_monte_carlo_amd.engine import Engine
    n = 40
    p, c = PR.pore_params(n=n)
    zones = [(0, -0.5 * p.R_oa, 0.0), (2, 0.25 * p.H, 0.5 * p.H)]
    rng = np.random.RandomState(9)
    t0 = np.empty((2, 263), dtype=object)
    for idx in np.ndindex(t0.shape):
        t0[idx] = int(rng.randint(0, 1000)) + (int(rng.randint(0, 2 ** 31)) << 64 if idx[1] % 5 == 0 else 0)
    t0[0, 0], t0[1, 4] = 2 ** 64 - 1, 2 ** 64 - 3                  # the next entry / inside count carries into the high word
    k = np.arange(n)
    x = np.where(k % 2 == 0, -0.2, 0.2) * p.R_oa
    z = np.where(k % 4 < 2, 0.3, 0.7) * p.H
    eng = Engine(p)
    eng.transit_config(TR.make_grid(zones, every=0))
    state = np.full(n, 1 | 1 << 4, dtype=np.uint32)              # everybody below both zones
    eng.transit_load(ints_to_words(t0), 9, state, None)
    tot, ns = eng.transit_read()
    assert ns == 9 and np.array_equal(tot, ints_to_words(t0))
    m = Mirror(zones, n)
    m.load(ints_to_words(t0), 9, state)
    eng.upload(x, np.zeros(n), z, np.zeros(n), np.zeros(n), np.zeros(n))
    eng.transit_sample()
    m.sample(x, np.zeros(n), z)
    t = m.check(eng)
    assert int(t[0, 0]) == 2 ** 64 - 1 + 20 and int(t[1, 4]) == 2 ** 64 - 3 + 20 and int(t[1, 0]) == int(t0[1, 0]) + 20
    with pytest.raises(ValueError):
        eng.transit_load(ints_to_words(t0)[:1], 0)
    with pytest.raises(ValueError):
        eng.transit_load(ints_to_words(t0), 0, state[:-1])
    eng.close()


# ---- 7. energised pore: host-RNG and device-RNG steps, and the host-free run ---------------------------------------------------
@pytest.mark.parametrize("device_rng", [False, True])
def test_energised_pore_run_equals_mirror_on_a_twin(device_rng):
    """Thin zones at the hot coating's lower edge, z = h_oa, on both sides of it.  run(k) samples after every step; the twin takes
    the same steps one at a time without the sampler, and the mirror sees its downloads."""
    def zones(p):
        return [(2, p.h_oa, p.h_oa + 0.5e-9), (2, p.h_oa - 1e-9, p.h_oa + 1e-9), (2, p.h_oa, p.z_gap_bottom)]
    steps = 10
    twin = SP.make_temp_sim(device_rng)
    m = Mirror(zones(twin.params), 20_000)
    for _ in range(steps):
        twin.timestep()
        m.add_state(twin.engine.download())
    state = twin.engine.download()
    twin.close()
    sim = SP.make_temp_sim(device_rng)
    sim.enable_transits(TR.make_grid(zones(sim.params)))
    sim.run(steps)
    t = m.check(sim.engine)
    assert m.n_samples == steps and sum(sum(_classes(t, k)) for k in range(3)) > 0 and all(int(t[k, 0:3].sum()) > 0 for k in range(3))
    st = sim.engine.download()
    for k in KEYS:
        assert np.array_equal(st[k], state[k]), k
    sim.close()


# ---- 12. the reduce at its shapes -------------------------------------------------------------------------------------------------
# a slab row's columns per zone (amc_transit.hip): the totals' with sum_tau2 as two columns, its low and its high 32-bit limb
TR_CLASS = REF.CLASS_COLUMNS + 1
TR_COLUMNS = 5 + 6 * TR_CLASS
_REDUCE_REF = {}


def _reduce_case(n_zones):
    """(params, zones, two states ten steps apart, the mirror after both), computed once"""
    if n_zones not in _REDUCE_REF:
        p, states = drifting_states(ODD_N, 11)
        zones = (_thin_zones(p) + [(0, -2e-9, 2e-9), (1, 0.0, 5e-9), (2, p.h_oa + 2e-9, p.h_oa + 4e-9), (0, 0.0, p.R_oa), (1, -p.R_oa, 0.0)])[:n_zones]
        m = Mirror(zones, ODD_N)
        for st in (states[0], states[10]):
            m.sample(*st[:3])
        _REDUCE_REF[n_zones] = (p, zones, (states[0], states[10]), m)
    return _REDUCE_REF[n_zones]


@pytest.mark.parametrize("blocks", ["1", "17", "33"])
@pytest.mark.parametrize("n_zones", [1, 8])
def test_reduce_shapes_equal_mirror(n_zones, blocks, monkeypatch):
    """One zone: W = 269 slab columns, five workgroups of the reduce; eight: W = 2,152.  1, 17 and 33 slab rows: below, one above
    and two above a multiple of the reduce's sixteen waves.  The second sample adds onto non-zero totals."""
    from argon_monte_carlo_amd.engine import Engine
    p, zones, states, m = _reduce_case(n_zones)
    assert n_zones * TR_COLUMNS == {1: 269, 8: 2152}[n_zones]
    monkeypatch.setenv("AMC_TRANSIT_BLOCKS", blocks)
    eng = Engine(p)
    eng.transit_config(TR.make_grid(zones, every=0))
    for st in states:
        eng.upload(*st)
        eng.transit_sample()
    t = m.check(eng)
    assert all(int(t[k, 0:3].sum()) > 0 for k in range(n_zones)) and sum(sum(_classes(t, k)) for k in range(n_zones)) > 0
    eng.close()


def test_reduce_adds_a_limb_pair_split_over_two_workgroups():
    """The reduce takes 64 slab columns per workgroup, and the thread of a sum_tau2 low-limb column adds the high limb's sum, the
    column beside it, into the same total.  Zone 4, exit class (entered from above, left above): the low limb is slab column 1215,
    lane 63 of workgroup 18, the high limb lane 0 of workgroup 19.  tau = 2^17 gives tau^2 = 2^34: a low limb of 0, a high limb of 4."""
    import re
    from argon_monte_carlo_amd import _lib
    from argon_monte_carlo_amd.sim import Simulation
    src = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "amc_transit.hip")).read()
    assert re.search(r"#define TR_CLASS \(AMC_TRANSIT_CLASS_COLUMNS \+ 1\)", src) and re.search(r"#define TR_COLUMNS \(5 \+ 6 \* TR_CLASS\)", src)
    zone, cls = 4, 2 * 1 + 1
    low = zone * TR_COLUMNS + 5 + cls * TR_CLASS + 2
    assert (TR_COLUMNS, TR_CLASS, low) == (269, 44, 1215) and low % 64 == 63
    n, who = 10, 3
    sim = Simulation("cube", n=n)
    L = float(sim.params.cube_x)
    zones = [(1, (0.1 + 0.1 * k) * L, (0.15 + 0.1 * k) * L) for k in range(8)]      # disjoint, in ascending order along y
    sim.enable_transits(TR.make_grid(zones), every=0)
    m = Mirror(zones, n)
    # everybody below every zone, but `who`: inside zone 4 since sample 0, entered from above — above zones 0 .. 3, below 5 .. 7
    state = np.full(n, 0x11111111, dtype=np.uint32)
    state[who] = 0x11100000 | (2 | 1 << 2) << 16 | 0x3333
    entry = np.zeros((8, n), dtype=np.uint32)
    zero = ints_to_words(np.zeros((8, REF.COLUMNS), dtype=object))
    ns = 2 ** 17
    sim.engine.transit_load(zero, ns, state, entry)
    m.load(zero, ns, state, entry)
    y = np.full(n, 0.05 * L)
    y[who] = 0.57 * L                   # above zone 4, still below zone 5: nobody else's position word changes
    m.sample(*_set_y(sim, n, L, y))
    sim.transits_sample()
    t = m.check(sim.engine)
    c = COL(1, 1)
    want = np.zeros((8, REF.COLUMNS), dtype=object)
    want[zone, c], want[zone, c + 1], want[zone, c + 2], want[zone, c + 3 + 17] = 1, 2 ** 17, 2 ** 34, 1
    assert np.array_equal(t, want), np.argwhere(t != want)
    sim.close()
