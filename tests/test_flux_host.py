"""CPU only: the sampled fluxes' host side — header, signatures and exports, known answers of the quantisers (tests/flux_ref.py
against a plain Python loop), the derived quantities on hand-made totals, and the grid limits."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from argon_monte_carlo_amd import _abi, _lib
from argon_monte_carlo_amd import fields as FL
from argon_monte_carlo_amd import fluxes as FX
from argon_monte_carlo_amd import params as PR
from tests import fields_ref as FREF
from tests import flux_ref as REF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["amc_flux_config", "amc_flux_sample", "amc_flux_read", "amc_flux_load", "amc_flux_reset"]
MASS, K_B = 6.63e-26, 1.380649e-23
UNIT = FX.make_grid("cartesian", (1, 1, 1), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))


# ---- header, signatures, library ------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_typed():
    main = open(os.path.join(ROOT, "include", "argonmc.h")).read()
    assert '#include "argonmc_flux.h"' in main
    assert os.path.join(ROOT, "include", "argonmc_flux.h") in _lib._source_files()
    hdr = open(os.path.join(ROOT, "include", "argonmc_flux.h")).read()
    lib = _lib.load()
    for name in NAMES:
        assert f"int {name}(amc_ctx *ctx" in hdr and hasattr(lib, name), name
    assert set(re.findall(r"^int (amc_[a-z_]+)\(", hdr, flags=re.M)) == set(_lib.FLUX_SIGNATURES) == set(NAMES)
    assert not set(_lib.FLUX_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.SHARD_SIGNATURES) | set(_lib.CORR_SIGNATURES))
    # argonmc.h itself still declares exactly SIGNATURES: the new contract is the included header's
    declared = set(re.findall(r"^(?:int|void|const char \*)\s*\*?\s*(amc_[a-z_]+)\s*\(", main, flags=re.M))
    assert declared == set(_lib.SIGNATURES) and not declared & set(NAMES)
    assert lib.amc_abi_version() == _abi.AMC_ABI_VERSION == 2
    mk = open(os.path.join(ROOT, "argon_monte_carlo_amd", "csrc", "Makefile")).read()
    assert "amc_fields.o" in mk and "argonmc_flux.h" in mk      # (the fluxes' entry points live beside the fields': one kernel template)


@pytest.mark.skipif(shutil.which("cc") is None, reason="no C compiler")
def test_flux_grid_layout_matches_header(tmp_path):
    src = tmp_path / "layout.c"
    names = ["struct_size", "kind", "n1", "n2", "n3", "reserved", "every", "step_offset", "lo", "hi"]
    body = "".join(f'    printf("{k} %zu\\n", offsetof(amc_flux_grid, {k}));\n' for k in names)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "argonmc.h"\nint main(void) {\n'
                   '    printf("sizeof %zu\\n", sizeof(amc_flux_grid));\n    printf("field %zu\\n", sizeof(amc_field_grid));\n' + body +
                   '    printf("max_bins %d\\n", AMC_FLUX_MAX_BINS);\n    printf("abi %d\\n", AMC_ABI_VERSION);\n'
                   '    printf("k_count %d\\n", AMC_K_COUNT);\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(line.rsplit(" ", 1) for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n") if line)
    assert int(out["sizeof"]) == C.sizeof(_abi.AmcFluxGrid) == int(out["field"]) == C.sizeof(_abi.AmcFieldGrid)
    for k in names:
        assert int(out[k]) == getattr(_abi.AmcFluxGrid, k).offset, k
    assert int(out["max_bins"]) == _abi.AMC_FLUX_MAX_BINS == 1024
    assert int(out["abi"]) == 2 and int(out["k_count"]) == len(_abi.AMC_K_NAMES) == 13      # no new kernel class


# ---- the quantisers ---------------------------------------------------------------------------------------------------------
def _loop_particle(c1, c2, c3):
    """the fourteen integers of one particle: Python floats, round() (half to even)"""
    e = (c1 * c1 + c2 * c2) + c3 * c3
    return [1, round(c1 * 2.0 ** 24), round(c2 * 2.0 ** 24), round(c3 * 2.0 ** 24),
            round((c1 * c1) * 2.0 ** 10), round((c2 * c2) * 2.0 ** 10), round((c3 * c3) * 2.0 ** 10),
            0, round((c1 * c2) * 2.0 ** 10), round((c1 * c3) * 2.0 ** 10), round((c2 * c3) * 2.0 ** 10),
            round(math.ldexp(e * c1, -6)), round(math.ldexp(e * c2, -6)), round(math.ldexp(e * c3, -6))]


def _q(c1, c2, c3):
    return [int(v) for v in REF.quantise([c1], [c2], [c3])[:, 0]]


def test_largest_values_in_range_stay_below_2_to_38():
    top = float(np.nextafter(2.0 ** 14, 0))
    for c in [(top, top, top), (-top, top, -top), (top, 0.0, 0.0)]:
        q = _q(*c)
        assert q == _loop_particle(*c)
        assert max(abs(v) for v in q[11:]) < 2 ** 38          # q3, the new quantiser: strictly below
        # the fields' q1 and q2 (and the cross products, the same format) ROUND UP to 2^38 at the very top of the range, as
        # they do in the sampled fields: "at most", and 2^24 such particles sum to at most 2^62, inside the signed 64-bit partial sums
        assert max(abs(v) for v in q) <= 2 ** 38
    q = _q(top, top, top)
    assert q[1] == q[4] == q[8] == 2 ** 38
    assert 2 ** 37 < q[11] == q[12] == q[13] <= 3 * 2 ** 36 < 2 ** 38     # e c / 64 just below 3 * 2^42 / 64, rounded
    assert 2 ** 24 * max(abs(v) for v in q) <= 2 ** 62 < 2 ** 63


def test_q3_rounds_ties_half_to_even():
    # c1 = 2^13 swallows the other squares: e = 2^26 exactly, so e c_k / 64 = m / 2 for c_k = m 2^-21
    u = 2.0 ** -21
    assert _q(2.0 ** 13, u, 5 * u)[11:] == [2 ** 33, 0, 2]              # 0.5 -> 0, 2.5 -> 2
    assert _q(2.0 ** 13, 3 * u, -7 * u)[11:] == [2 ** 33, 2, -4]        # 1.5 -> 2, -3.5 -> -4
    assert _q(2.0 ** 13, -u, -3 * u)[11:] == [2 ** 33, 0, -2]
    assert _q(4.0, 6.0, 2.0)[11:] == [4, 5, 2]                          # e = 56: 3.5 -> 4, 5.25 -> 5, 1.75 -> 2
    assert _q(4.0, 2.0, 2.0)[11:] == [2, 1, 1]                          # e = 24: 1.5 -> 2, 0.75 -> 1
    # the cross products' ties
    assert _q(1.0, 2.0 ** -11, 3 * 2.0 ** -11)[8:11] == [0, 2, 0] and _q(5.0, -(2.0 ** -11), 1.0)[8:11] == [-2, 5120, -0]


def test_e_is_summed_in_the_order_written():
    # s1 = 2^26 (ulp 2^-26); s2 = s3 = 161^2 2^-42 = 1.58 * 2^-28: each alone is below half an ulp of s1, their sum is above
    c1, c2 = 2.0 ** 13, 161 * 2.0 ** -21
    s1, s2 = c1 * c1, c2 * c2
    assert (s1 + s2) + s2 == s1 and s1 + (s2 + s2) == s1 + 2.0 ** -26
    assert round(math.ldexp(((s1 + s2) + s2) * c2, -6)) == 80           # 80.5 exactly: the tie goes to even
    assert round(math.ldexp((s1 + (s2 + s2)) * c2, -6)) == 81           # the other order is above the tie
    assert _q(c1, c2, c2)[12:] == [80, 80] == _loop_particle(c1, c2, c2)[12:]


def test_reference_equals_plain_loop_on_random_states():
    rng = np.random.default_rng(5)
    for g in (FX.make_grid("cartesian", (3, 2, 4), (0.0, -1e-7, 2e-8), (1e-7, 1e-7, 3e-7)),
              FX.make_grid("axisymmetric", (2, 9), (0.0, 0.0), (1.5e-7, 3.2e-6))):
        n = 300
        lo, hi = np.array(g.lo), np.array(g.hi)
        if g.kind == FX.AMC_FIELDS_CARTESIAN:
            pos = rng.uniform(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), size=(n, 3))
        else:
            r, th = rng.uniform(0, 1.1 * hi[0], n), rng.uniform(0, 2 * np.pi, n)
            pos = np.stack([r * np.cos(th), r * np.sin(th), rng.uniform(-0.1 * hi[1], 1.1 * hi[1], n)], axis=1)
        pos[0, :2] = 0.0                    # on the axis
        vel = rng.normal(scale=300.0, size=(n, 3))
        got, outside = REF.sample(g, *pos.T, *vel.T)
        b, c1, c2, c3 = FREF.bins_and_components(g, *pos.T, *vel.T)
        want = [[0] * 14 for _ in range(FX.grid_bins(g))]
        for p in range(n):
            if b[p] >= 0:
                want[b[p]] = [s + v for s, v in zip(want[b[p]], _loop_particle(float(c1[p]), float(c2[p]), float(c3[p])))]
        assert outside == int((b < 0).sum()) >= 3
        assert [[int(v) for v in row.ravel()] for row in got] == want
        # row A is the fields' reference, row B's first entry is never added to
        fa, fo = FREF.sample(FL.copy_grid(g), *pos.T, *vel.T)
        assert fo == outside and (got[:, 0, :] == fa).all() and all(int(v) == 0 for v in got[:, 1, 0])


@pytest.mark.parametrize("value", [2.0 ** 14, -(2.0 ** 14), float("nan"), float("inf")])
def test_values_on_the_range_limit_are_reported_not_summed(value):
    pos = np.full((3, 6), 0.5)
    vel = np.tile(np.array([[10.0], [20.0], [30.0]]), (1, 6))
    vel[2, 4] = vel[1, 2] = value           # two offenders: the lowest index is named
    with pytest.raises(REF.RangeError) as e:
        REF.sample(UNIT, *pos, *vel)
    assert e.value.index == 2
    pos[0, [2, 4]] = 1.5                    # outside the grid they are only counted
    got, out = REF.sample(UNIT, *pos, *vel)
    assert out == 2 and int(got[0, 0, 0]) == 4


# ---- derive on hand-made totals -----------------------------------------------------------------------------------------------
def _totals(vels):
    """integer totals of one bin holding the particles ``vels`` (rows of c1, c2, c3)"""
    v = np.asarray(vels, dtype=np.float64)
    return np.array([[int(s) for s in REF.quantise(*v.T).sum(axis=1)]], dtype=object).reshape(1, 2, 7)


def test_one_velocity_gives_zero_stress_and_zero_heat_flux_exactly():
    c = (120.0, -80.0, 304.0)               # multiples of 8: e c / 64 is an integer, every quantised value is exact
    f = FX.derive(UNIT, FX.ints_to_words(_totals([c] * 5)), 1, 0, MASS, K_B)
    assert f["count"].tolist() == [5] and f["number_density"][0] == 5.0
    assert f["velocity"][0].tolist() == list(c)
    assert (f["pressure_tensor"][0] == 0.0).all() and f["pressure"][0] == 0.0 and f["T"][0] == 0.0
    assert (f["heat_flux"][0] == 0.0).all()
    e = c[0] * c[0] + c[1] * c[1] + c[2] * c[2]
    assert f["energy_flux"][0].tolist() == [5.0 * MASS / 2 * (e * k) for k in c]


def test_a_pair_of_opposite_velocities_gives_the_normal_stress_and_no_heat_flux():
    v = 250.0
    for axis in range(3):
        c = [0.0, 0.0, 0.0]
        c[axis] = v
        f = FX.derive(UNIT, FX.ints_to_words(_totals([c, [-k for k in c]])), 2, 0, MASS, K_B)
        nd = 2 / (2 * 1.0)
        assert f["number_density"][0] == nd and f["velocity"][0].tolist() == [0.0, 0.0, 0.0]
        want = np.zeros((3, 3))
        want[axis, axis] = nd * MASS * (v * v)
        assert (f["pressure_tensor"][0] == want).all()
        assert f["pressure"][0] == want[axis, axis] / 3 and f["T"][0] == want[axis, axis] / 3 / (nd * K_B)
        assert (f["heat_flux"][0] == 0.0).all() and (f["energy_flux"][0] == 0.0).all()


def test_a_skewed_triple_gives_the_heat_flux_computed_by_hand():
    vels = [(8.0, 16.0, 24.0), (8.0, 16.0, -8.0), (-16.0, 40.0, 32.0)]      # multiples of 8: every quantised value is exact
    f = FX.derive(UNIT, FX.ints_to_words(_totals(vels)), 1, 0, MASS, K_B)
    # by hand, straight from the definition: u = <c>, C = c - u, P_ab = nd m <C_a C_b>, q_a = nd m / 2 <|C|^2 C_a>
    fr = [[Fraction(k) for k in c] for c in vels]
    u = [sum(c[a] for c in fr) / 3 for a in range(3)]
    assert u == [0, 24, 16]
    Cs = [[c[a] - u[a] for a in range(3)] for c in fr]
    assert Cs == [[8, -8, 8], [8, -8, -24], [-16, 16, 16]]
    P = [[sum(C[a] * C[b] for C in Cs) / 3 for b in range(3)] for a in range(3)]
    q = [sum((C[0] ** 2 + C[1] ** 2 + C[2] ** 2) * C[a] for C in Cs) / 3 for a in range(3)]
    assert P == [[128, -128, -128], [-128, 128, 128], [-128, 128, Fraction(896, 3)]] and q == [-Fraction(5120, 3), Fraction(5120, 3), -1024]
    nd = 3.0
    assert f["velocity"][0].tolist() == [0.0, 24.0, 16.0]
    assert f["pressure_tensor"][0].tolist() == [[nd * MASS * float(P[a][b]) for b in range(3)] for a in range(3)]
    assert f["heat_flux"][0].tolist() == [nd * MASS / 2 * float(q[a]) for a in range(3)]
    assert (f["pressure_tensor"][0] == f["pressure_tensor"][0].T).all()
    F = [sum((c[0] ** 2 + c[1] ** 2 + c[2] ** 2) * c[a] for c in fr) / 3 for a in range(3)]
    assert f["energy_flux"][0].tolist() == [nd * MASS / 2 * float(F[a]) for a in range(3)]


def test_derive_equals_the_reference_on_random_integer_totals():
    g = FX.make_grid("axisymmetric", (3, 4), (0.0, 0.0), (1.5e-7, 3.2e-6))
    rng = np.random.default_rng(11)
    sums = np.empty((12, 2, 7), dtype=object)
    for b in range(12):
        n = int(rng.integers(0, 4)) if b < 4 else int(rng.integers(2, 10 ** 6)) * (10 ** 9 if b == 11 else 1)    # (bin 11: beyond 64 bits)
        v = rng.normal(scale=400.0, size=3)
        sums[b, 0] = [n] + [int(n * v[a] * 2 ** 24 + rng.integers(-2 ** 30, 2 ** 30)) for a in range(3)] + \
                     [int(n * (v[a] ** 2 + 9e4) * 2 ** 10 + rng.integers(-2 ** 30, 2 ** 30)) for a in range(3)]
        sums[b, 1] = [0] + [int(n * v[a] * v[c] * 2 ** 10 + rng.integers(-2 ** 30, 2 ** 30)) for a, c in ((0, 1), (0, 2), (1, 2))] + \
                     [int(n * v[a] * 5e5 / 64 + rng.integers(-2 ** 30, 2 ** 30)) for a in range(3)]
        if n == 0:
            sums[b] = 0
    assert max(abs(int(v)) for v in sums.ravel()) > 2 ** 64
    f = FX.derive(g, FX.ints_to_words(sums), 7, 3, MASS, K_B)
    want = REF.derive(g, sums, 7, MASS, K_B)
    for k, w in want.items():
        assert np.array_equal(f[k], w, equal_nan=True), k
    few = [b for b in range(12) if int(sums[b, 0, 0]) < 2]
    assert few and all(np.isnan(f[k][few]).all() for k in ("velocity", "pressure_tensor", "pressure", "T", "energy_flux", "heat_flux"))
    assert np.isfinite(f["heat_flux"][4:]).all() and (f["number_density"][4:] > 0).all()
    assert (f["n_samples"], f["n_outside"], f["shape"], f["totals"].shape) == (7, 3, (3, 4, 1), (12, 2, 7, 2))
    assert f["count"].tolist() == [int(sums[b, 0, 0]) for b in range(12)]


# ---- grids ------------------------------------------------------------------------------------------------------------------
def test_1024_bins_are_accepted_and_1025_refused():
    g = FX.make_grid("cartesian", (16, 8, 8), (0, 0, 0), (1, 1, 1), every=3)
    assert FX.grid_bins(g) == 1024 == _abi.AMC_FLUX_MAX_BINS and FX.totals_shape(g) == (1024, 2, 7, 2)
    assert isinstance(g, _abi.AmcFluxGrid) and (g.struct_size, g.every, g.reserved) == (C.sizeof(_abi.AmcFluxGrid), 3, 0)
    assert FX.grid_bins(FX.make_grid("axisymmetric", (8, 128), (0, 0), (1, 1))) == 1024
    for n in [(1025, 1, 1), (41, 5, 5), (16, 8, 9)]:
        with pytest.raises(ValueError):
            FX.make_grid("cartesian", n, (0, 0, 0), (1, 1, 1))
    with pytest.raises(ValueError):
        FX.make_grid("axisymmetric", (5, 205), (0, 0), (1, 1))
    with pytest.raises(ValueError):         # a fields grid beyond the fluxes' limit does not convert either
        FX.grid_from_array(FL.grid_to_array(FL.make_grid("cartesian", (2048, 1, 1), (0, 0, 0), (1, 1, 1))))
    h = FX.copy_grid(g, every=5, step_offset=7)
    assert isinstance(h, _abi.AmcFluxGrid) and (h.every, h.step_offset, g.every) == (5, 7, 3)


def test_default_grids_and_checkpoint_arrays():
    pc, _ = PR.cube_params_for_n(1000)
    g = FX.default_grid(pc)
    assert (g.kind, g.n1, g.n2, g.n3, g.every) == (FX.AMC_FIELDS_CARTESIAN, 8, 8, 8, 0)
    assert list(g.lo) == [0.0, 0.0, 0.0] and list(g.hi) == [pc.cube_x, pc.cube_y, pc.cube_z]
    for energised in (False, True):
        pp, _ = PR.pore_params(n=1000, energised=energised)
        g = FX.default_grid(pp, every=5)
        assert (g.kind, g.n1, g.n2, g.n3, g.every) == (FX.AMC_FIELDS_AXISYMMETRIC, 8, 128, 1, 5)
        assert (g.lo[0], g.hi[0], g.lo[1], g.hi[1]) == (0.0, pp.R_oa, 0.0, pp.H)
    h = FX.grid_from_array(FX.grid_to_array(FX.copy_grid(g, step_offset=9)))
    assert isinstance(h, _abi.AmcFluxGrid) and bytes(h) == bytes(FX.copy_grid(g, step_offset=9))
    assert len(FX.QUANTITIES) == 2 and all(len(r) == 7 for r in FX.QUANTITIES) and FX.QUANTITIES[0] == tuple(
        q.replace("q2_c1", "q2_c1c1").replace("q2_c2", "q2_c2c2").replace("q2_c3", "q2_c3c3") for q in FL.QUANTITIES)
