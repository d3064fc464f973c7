"""CPU only: the sampled transits' host side — header, signatures and exports, the grid's layout and limits, the default zones,
the derived quantities on hand-made totals, and the mirror (tests/transit_ref.py): against a plain per-particle Python loop on
crafted sequences, its invariants on a drifting state, and the entry rate of a collisionless gas against kinetic theory."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from argon_monte_carlo_amd import _abi, _lib
from argon_monte_carlo_amd import ic as IC
from argon_monte_carlo_amd import params as PR
from argon_monte_carlo_amd import transits as TR
from argon_monte_carlo_amd.totals import ints_to_words, words_to_ints
from tests import transit_ref as REF
from tests.sampler_states import ODD_N, drifting_states

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["amc_transit_config", "amc_transit_sample", "amc_transit_read", "amc_transit_state", "amc_transit_load", "amc_transit_reset"]


# ---- header, signatures, library ------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_typed():
    main = open(os.path.join(ROOT, "include", "argonmc.h")).read()
    assert '#include "argonmc_transit.h"' in main
    assert os.path.join(ROOT, "include", "argonmc_transit.h") in _lib._source_files()
    hdr = open(os.path.join(ROOT, "include", "argonmc_transit.h")).read()
    lib = _lib.load()
    for name in NAMES:
        assert f"int {name}(amc_ctx *ctx" in hdr and hasattr(lib, name), name
        assert getattr(lib, name).argtypes == _lib.TRANSIT_SIGNATURES[name][1]
    assert set(re.findall(r"^int (amc_[a-z_]+)\(", hdr, flags=re.M)) == set(_lib.TRANSIT_SIGNATURES) == set(NAMES)
    others = (set(_lib.SIGNATURES) | set(_lib.SHARD_SIGNATURES) | set(_lib.CORR_SIGNATURES) | set(_lib.FLUX_SIGNATURES) |
              set(_lib.MFP_SIGNATURES) | set(_lib.VDF_SIGNATURES))
    assert not set(NAMES) & others
    assert lib.amc_abi_version() == _abi.AMC_ABI_VERSION == 2
    mk = open(os.path.join(ROOT, "argon_monte_carlo_amd", "csrc", "Makefile")).read()
    assert "amc_transit.o" in mk and "argonmc_transit.h" in mk


@pytest.mark.skipif(shutil.which("cc") is None, reason="no C compiler")
def test_transit_grid_layout_matches_header(tmp_path):
    src = tmp_path / "layout.c"
    names = ["struct_size", "n_zones", "every", "step_offset", "axis", "lo", "hi", "reserved"]
    consts = {"max_zones": "AMC_TRANSIT_MAX_ZONES", "hist": "AMC_TRANSIT_HIST", "class_columns": "AMC_TRANSIT_CLASS_COLUMNS",
              "columns": "AMC_TRANSIT_COLUMNS", "abi": "AMC_ABI_VERSION", "k_count": "AMC_K_COUNT"}
    body = "".join(f'    printf("{k} %zu\\n", offsetof(amc_transit_grid, {k}));\n' for k in names)
    body += "".join(f'    printf("{k} %d\\n", (int){v});\n' for k, v in consts.items())
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "argonmc.h"\nint main(void) {\n'
                   '    printf("sizeof %zu\\n", sizeof(amc_transit_grid));\n' + body +
                   '    printf("max_samples %lld\\n", (long long)AMC_TRANSIT_MAX_SAMPLES);\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(line.rsplit(" ", 1) for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n") if line)
    assert int(out["sizeof"]) == C.sizeof(_abi.AmcTransitGrid) == 200
    for k in names:
        assert int(out[k]) == getattr(_abi.AmcTransitGrid, k).offset, k
    assert int(out["max_zones"]) == _abi.AMC_TRANSIT_MAX_ZONES == 8 and int(out["hist"]) == _abi.AMC_TRANSIT_HIST == 40
    assert int(out["class_columns"]) == _abi.AMC_TRANSIT_CLASS_COLUMNS == 43 == REF.CLASS_COLUMNS
    assert int(out["columns"]) == _abi.AMC_TRANSIT_COLUMNS == 263 == REF.COLUMNS == 5 + 6 * 43
    assert int(out["max_samples"]) == _abi.AMC_TRANSIT_MAX_SAMPLES == REF.MAX_SAMPLES == 2 ** 32 - 1
    assert int(out["abi"]) == 2 and int(out["k_count"]) == len(_abi.AMC_K_NAMES) == 13      # no new kernel class


# ---- the grid limits ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [
    {"zones": []}, {"zones": [(0, 0.0, 1.0)] * 9}, {"zones": [(3, 0.0, 1.0)]}, {"zones": [(-1, 0.0, 1.0)]}, {"zones": [(0, 1.0, 1.0)]},
    {"zones": [(0, 2.0, 1.0)]}, {"zones": [(0, 0.0, math.inf)]}, {"zones": [(0, -math.inf, 0.0)]}, {"zones": [(0, math.nan, 1.0)]},
    {"zones": [(0, 0.0, 1.0)], "reserved": (0, 1)}, {"zones": [(0, 0.0, 1.0)], "reserved": (7, 0)}, {"zones": [(0, 0.0, 1.0)], "every": -1},
    {"zones": [(0, 0.0, 1.0)], "step_offset": -1}])
def test_make_grid_refuses_what_the_library_would(kw):
    with pytest.raises(ValueError):
        TR.make_grid(**kw)


def test_make_grid_accepts_the_limits_and_round_trips():
    g = TR.make_grid([(k % 3, -1.0 - k, 2.5 + k) for k in range(8)], every=4, step_offset=9)
    assert (g.n_zones, g.every, g.step_offset, g.struct_size) == (8, 4, 9, 200) and list(g.axis) == [0, 1, 2, 0, 1, 2, 0, 1]
    assert TR.zones(g)[7] == (1, -8.0, 9.5) and TR.totals_shape(g) == (8, 263, 2)
    a = TR.grid_to_array(g)
    assert a.dtype == np.float64 and a.shape == (27,) and bytes(TR.grid_from_array(a)) == bytes(g)
    one = TR.make_grid([("z", 0.0, float(np.nextafter(0.0, 1.0)))], every=0)
    assert (one.n_zones, one.axis[0], one.every) == (1, 2, 0) and list(one.axis[1:]) == [0] * 7 and list(one.hi[1:]) == [0.0] * 7
    assert bytes(TR.grid_from_array(TR.grid_to_array(one))) == bytes(one)
    c = TR.copy_grid(g, every=0, step_offset=3)
    assert (c.every, c.step_offset, g.every, g.step_offset) == (0, 3, 4, 9)
    with pytest.raises(ValueError):
        TR.copy_grid(g, every=-2)


def test_default_grids():
    p, _ = PR.cube_params(n=1000)
    g = TR.default_grid(p)
    L = p.cube_x
    assert g.every == 1 and TR.zones(g) == [(0, 0.0, L / 3.0), (0, L / 3.0, 2.0 * L / 3.0), (0, 2.0 * L / 3.0, L)]
    for energised in (False, True):
        p, _ = PR.pore_params(n=1000, energised=energised)
        g = TR.default_grid(p, every=5)
        assert g.every == 5 and TR.zones(g) == [(2, p.h_oa, p.z_cold), (2, p.h_oa, p.z_gap_bottom), (2, p.z_gap_bottom, p.z_gap_top),
                                                (2, p.z_gap_top, p.z_cold)]
        assert p.h_oa < p.z_gap_bottom < p.z_gap_top < p.z_cold


# ---- derived quantities on hand-written totals -------------------------------------------------------------------------------
def test_derive_on_hand_written_totals():
    g = TR.make_grid([(2, 0.0, 1.0), (0, -1.0, 1.0)], every=4)
    t = np.zeros((2, 263), dtype=object)
    z = t[0]
    z[0], z[1], z[2], z[3], z[4] = 40, 12, 5, 2, 300            # entries from below, above, already inside; skipped; inside_sum
    c = TR.class_column
    z[c(0, 1)], z[c(0, 1, 1)], z[c(0, 1, 2)] = 10, 50, 290       # from below, out above: tau 5 on average, variance 4
    z[c(0, 1, 3 + 2)] = 10
    z[c(0, 0)], z[c(0, 0, 1)], z[c(0, 0, 2)] = 30, 30, 30        # from below, back below: every tau = 1
    z[c(0, 0, 3)] = 30
    z[c(1, 0)], z[c(1, 0, 1)], z[c(1, 0, 2)] = 3, 3 * 2 ** 33, 3 * 2 ** 66     # from above, out below: tau = 2^33 (a 128-bit sum)
    z[c(1, 0, 3 + 33)] = 3
    z[c(1, 1)], z[c(1, 1, 1)], z[c(1, 1, 2)] = 9, 18, 36
    z[c(2, 1)], z[c(2, 1, 1)], z[c(2, 1, 2)] = 4, 12, 40
    dt = 0.5
    d = TR.derive(g, ints_to_words(t), 100, dt)
    iv = 4 * dt
    assert d["interval"] == iv and d["n_samples"] == 100
    assert d["transmission"][0].tolist() == [0.25, 0.25] and d["return_probability"][0].tolist() == [0.75, 0.75]
    assert d["transmission_err"][0, 0] == math.sqrt(0.25 * 0.75 / 40) and d["transmission_err"][0, 1] == math.sqrt(0.25 * 0.75 / 12)
    assert d["residence_mean"][0, 0, 1] == 5.0 * iv and d["residence_var"][0, 0, 1] == 4.0 * iv * iv
    assert d["residence_mean"][0, 0, 0] == iv and d["residence_var"][0, 0, 0] == 0.0
    assert d["residence_mean"][0, 1, 0] == 2.0 ** 33 * iv and d["residence_var"][0, 1, 0] == 0.0
    assert d["residence_mean"][0, 2, 1] == 3.0 * iv and d["residence_var"][0, 2, 1] == 1.0 * iv * iv
    assert np.isnan(d["residence_mean"][0, 2, 0]) and np.isnan(d["residence_var"][0, 2, 0])
    T = 100 * iv
    assert d["entry_rate"][0].tolist() == [40 / T, 12 / T, 5 / T] and d["exit_rate"][0].tolist() == [33 / T, 23 / T]
    assert d["occupancy"][0] == 3.0 and d["little_residence"][0] == 3.0 / (33 / T + 23 / T)
    assert d["inside_now"].tolist() == [57 - 56, 0] and d["skipped"].tolist() == [2, 0] and d["count"][0].tolist() == [[30, 10], [3, 9], [0, 4]]
    assert d["hist"].shape == (2, 3, 2, 40) and d["hist"][0, 0, 1, 2] == 10 and d["hist"][0, 1, 0, 33] == 3 and d["hist"].sum() == 43
    assert d["hist_edges"][:3].tolist() == [1.0, 2.0, 4.0] and d["hist_edges"].shape == (41,) and math.isinf(d["hist_edges"][40])
    assert d["hist_edges_s"][5] == 32.0 * iv
    # the empty zone: NaN probabilities and residences, zero rates, occupancy 0, no Little's-law residence
    assert np.isnan(d["transmission"][1]).all() and np.isnan(d["return_probability"][1]).all() and np.isnan(d["residence_mean"][1]).all()
    assert d["entry_rate"][1].tolist() == [0.0, 0.0, 0.0] and d["occupancy"][1] == 0.0 and np.isnan(d["little_residence"][1])
    # without samples nothing has a rate; samples taken by hand count as one step each unless told otherwise
    e = TR.derive(TR.copy_grid(g, every=0), ints_to_words(t), 0, dt)
    assert e["interval"] == dt and np.isnan(e["entry_rate"]).all() and np.isnan(e["occupancy"]).all()
    assert TR.derive(TR.copy_grid(g, every=0), ints_to_words(t), 10, dt, every=6)["interval"] == 6 * dt
    assert np.array_equal(TR.split(g, ints_to_words(t))["sum_tau2"][0, 1, 0], 3 * 2 ** 66)


# ---- the mirror against a plain per-particle loop ---------------------------------------------------------------------------------
def _loop(zones, frames):
    """The header's table, one particle and one zone at a time: (totals as Python ints, state words, entry indices)."""
    n = len(frames[0][0])
    tot = [[0] * 263 for _ in zones]
    pos = [[0] * n for _ in zones]
    side = [[0] * n for _ in zones]
    entry = [[0] * n for _ in zones]
    for s, frame in enumerate(frames):
        for k, (axis, lo, hi) in enumerate(zones):
            for p in range(n):
                u = float(frame[axis][p])
                b = 1 if u < lo else 2 if u < hi else 3
                a = pos[k][p]
                if b == 2 and a != 2:
                    side[k][p] = 2 if a == 0 else 0 if a == 1 else 1
                    tot[k][side[k][p]] += 1
                    entry[k][p] = s
                elif a == 2 and b != 2:
                    tau = s - entry[k][p]
                    assert tau >= 1
                    c = 5 + 43 * (2 * side[k][p] + (0 if b == 1 else 1))
                    tot[k][c] += 1
                    tot[k][c + 1] += tau
                    tot[k][c + 2] += tau * tau
                    tot[k][c + 3 + min(int(math.floor(math.log2(tau))), 39)] += 1
                    side[k][p] = 0
                elif a in (1, 3) and b in (1, 3) and a != b:
                    tot[k][3] += 1
                pos[k][p] = b
                if b == 2:
                    tot[k][4] += 1
    state = [sum((pos[k][p] | side[k][p] << 2) << (4 * k) for k in range(len(zones))) for p in range(n)]
    return tot, state, entry


def test_mirror_equals_a_plain_loop_on_crafted_sequences():
    rng = np.random.RandomState(5)
    zones = [(0, 0.0, 1.0), (0, 0.25, 0.5), (1, -1.0, 0.0), (2, 0.5, 3.0), (0, 0.0, 0.25)]      # overlapping, nested, abutting, three axes
    n = 37
    # a slow random walk (residences of many samples), with jumps now and then (skipped crossings, entries from both sides) ...
    x = rng.uniform(-0.5, 1.5, n)
    frames = []
    for s in range(90):
        x = x + rng.normal(0.0, 0.08, n)
        jump = rng.rand(n) < 0.03
        x = np.where(jump, rng.uniform(-1.0, 2.0, n), x)
        frames.append((x.copy(), rng.uniform(-2.0, 1.0, n) if s % 7 == 0 else x - 0.7, 2.0 * x + 0.5))
    # ... and values on the bounds themselves
    edge = np.resize(np.array([0.0, 1.0, np.nextafter(0.0, -1.0), np.nextafter(1.0, 0.0), 0.25, 0.5, np.nextafter(0.25, 0.0), -0.0]), n)
    frames.insert(40, (edge, edge - 1.0, edge + 0.5))
    tot, state, entry = _loop(zones, frames)
    m = REF.Mirror(zones, n)
    for f in frames:
        m.sample(*f)
    assert m.n_samples == 91 and m.tot == tot
    assert m.state.tolist() == state
    inside = [[((w >> (4 * k)) & 3) == 2 for w in state] for k in range(len(zones))]
    for k in range(len(zones)):
        assert [int(v) for v, i in zip(m.entry[k], inside[k]) if i] == [v for v, i in zip(entry[k], inside[k]) if i]
    t = np.array(tot, dtype=object)
    assert all(t[k, 3] > 0 and t[k, 0] > 0 and t[k, 1] > 0 and t[k, 2] > 0 for k in range(5)), t[:, :5]
    assert sum(int(t[0, TR.class_column(e, x)]) > 0 for e in range(3) for x in range(2)) == 6
    assert np.array_equal(words_to_ints(m.words()), t)
    # the edge frame: u == lo is inside, u == hi above, nextafter(lo, -inf) below, -0.0 == lo inside
    b = REF.positions(edge[:8], 0.0, 1.0).tolist()
    assert b == [2, 3, 1, 2, 2, 2, 2, 2]
    assert REF.positions(edge[:8], 0.25, 0.5).tolist() == [1, 3, 1, 3, 2, 3, 1, 1]


def test_mirror_stops_at_a_nan_and_at_the_sample_limit():
    zones = [(1, 0.0, 1.0)]
    m = REF.Mirror(zones, 4)
    y = np.array([0.5, 0.5, -1.0, 2.0])
    nan_x = np.full(4, math.nan)
    m.sample(nan_x, y, nan_x)                   # axes nobody looks at may hold anything
    assert m.bad is None and m.n_samples == 1 and m.tot[0][2] == 2 and m.tot[0][4] == 2
    y2 = y.copy()
    y2[1] = y2[3] = math.nan
    m.sample(nan_x, y2, nan_x)
    assert m.bad == 1 and m.n_samples == 1 and m.tot[0][4] == 2
    m.sample(nan_x, y, nan_x)
    assert m.n_samples == 1
    # the limit: sample number 2^32 - 1 (index 2^32 - 2) is the last one
    m = REF.Mirror(zones, 2)
    t = np.zeros((1, 263), dtype=object)
    t[0, 2] = 2
    m.load(ints_to_words(t), 2 ** 32 - 2, state=np.array([2 | 2 << 2, 2 | 2 << 2], dtype=np.uint32), entry=np.array([[0, 5]], dtype=np.uint32))
    m.sample(nan_x[:2], np.array([-1.0, 0.5]), nan_x[:2])
    c = TR.class_column(2, 0)
    tau = 2 ** 32 - 2
    assert m.n_samples == 2 ** 32 - 1 and not m.over and m.tot[0][c:c + 3] == [1, tau, tau * tau] and m.tot[0][c + 3 + 31] == 1
    before = [list(r) for r in m.tot]
    m.sample(nan_x[:2], np.array([-1.0, 2.0]), nan_x[:2])
    assert m.over and m.n_samples == 2 ** 32 - 1 and m.tot == before and m.state.tolist() == [1, 2 | 2 << 2]


# ---- invariants on a drifting state ----------------------------------------------------------------------------------------------
def test_mirror_invariants_on_a_drifting_state():
    samples = 40
    p, states = drifting_states(ODD_N, samples)
    zones = [(2, p.h_oa, p.h_oa + 0.5e-9), (2, p.h_oa, p.h_oa + 2e-9), (2, 0.0, 1e-9), (0, -2e-9, 2e-9), (2, p.h_oa, p.z_cold)]
    m = REF.Mirror(zones, ODD_N)
    for st in states:
        m.sample(*st[:3])
    assert m.n_samples == samples
    t = np.array(m.tot, dtype=object)
    for k in range(len(zones)):
        exits = sum(int(t[k, TR.class_column(e, x)]) for e in range(3) for x in range(2))
        assert int(t[k, 0:3].sum()) - exits == m.inside_counts[-1][k] == int((((m.state >> np.uint32(4 * k)) & np.uint32(3)) == 2).sum())
        assert int(t[k, 4]) == sum(c[k] for c in m.inside_counts)
        for e in range(3):
            for x in range(2):
                c = TR.class_column(e, x)
                assert int(t[k, c]) == int(t[k, c + 3:c + 43].sum())
                assert int(t[k, c]) <= int(t[k, c + 1]) <= int(t[k, c + 2])        # tau >= 1
    assert all(int(t[k, 0]) + int(t[k, 1]) > 0 for k in range(4)), t[:, :5]
    assert sum(int(t[k, TR.class_column(e, x)]) for k in range(4) for e in range(3) for x in range(2)) > 0
    d = TR.derive(TR.make_grid(zones), m.words(), m.n_samples, 1e-12)
    assert d["inside_now"].tolist() == m.inside_counts[-1]
    assert np.allclose(d["occupancy"], np.mean(np.array(m.inside_counts), axis=0), rtol=1e-15)


# ---- one physical check: the entry rate of a collisionless gas -----------------------------------------------------------------------
def test_entries_into_the_middle_third_match_the_kinetic_wall_flux():
    """A collisionless gas in the specular cube (x only: free flight, mirrored at 0 and cube_x), N = 1,000 Maxwell atoms from
    ic.cube_ic, a sample of the start and one after each of 60 steps.  Kinetic theory puts n v_mean / 4 atoms per area and time
    through a plane from one side, so each face of the middle third sees N / cube_x * v_mean / 4 * 60 dt entries, v_mean =
    a_shape sqrt(8 / pi); the count is Poisson-like: five standard deviations of the expectation are allowed."""
    n, steps = 1000, 60
    p, c = PR.cube_params(n=n)
    x, y, z, vx, vy, vz = IC.cube_ic(p, c, 21)
    L, dt = float(p.cube_x), float(c["dt"])
    g = TR.default_grid(p)
    m = REF.Mirror(TR.zones(g), n)
    x, vx = x.copy(), vx.copy()
    m.sample(x, y, z)
    for _ in range(steps):
        x = x + dt * vx
        lo, hi = x < 0.0, x > L
        x = np.where(lo, -x, np.where(hi, 2.0 * L - x, x))
        vx = np.where(lo | hi, -vx, vx)
        assert ((x >= 0.0) & (x <= L)).all()
        m.sample(x, y, z)
    v_mean = float(c["a_shape"]) * math.sqrt(8.0 / math.pi)
    expect = n / L * v_mean / 4.0 * steps * dt
    mid = m.tot[1]
    taus = [j for e in range(3) for s in range(2) for j in range(40) if mid[TR.class_column(e, s, 3 + j)]]
    print("expected per face", expect, "entries from below / above", mid[0], mid[1], "skipped", mid[3], "histogram columns", min(taus), max(taus))
    assert expect >= 300.0
    for face in (0, 1):
        assert abs(mid[face] - expect) < 5.0 * math.sqrt(expect), (face, mid[face], expect)
    # the outer thirds have a wall behind them: whoever comes in from the middle goes back there
    lo3, hi3 = m.tot[0], m.tot[2]
    assert lo3[0] == 0 and hi3[1] == 0 and lo3[TR.class_column(1, 0)] == 0 and hi3[TR.class_column(0, 1)] == 0
    assert lo3[TR.class_column(1, 1)] > 0 and hi3[TR.class_column(0, 0)] > 0
    d = TR.derive(g, m.words(), m.n_samples, dt)
    # ... and without collisions nobody turns round inside the middle third
    assert d["transmission"][1].tolist() == [1.0, 1.0] and d["transmission"][0, 1] == 0.0 and d["return_probability"][2, 0] == 1.0
