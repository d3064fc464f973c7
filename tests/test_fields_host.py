"""CPU only: the sampled fields' host side — the NumPy reference (tests/fields_ref.py) against a plain Python loop, the
128-bit words, the derived fields, the ctypes mirror of amc_field_grid and the grid validation."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from argon_monte_carlo_amd import _abi
from argon_monte_carlo_amd import fields as FL
from argon_monte_carlo_amd import params as PR
from tests import fields_ref as REF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference against a plain loop ------------------------------------------------------------------------------------
def _loop_axis(u, lo, hi, n):
    w = (hi - lo) / n
    v = (u - lo) / w
    if v != v:
        return -1
    i = math.floor(v)
    if i == n and u <= hi:
        return n - 1
    return i if 0 <= i < n else -1


def _loop_sample(g, parts):
    bins = g.n1 * g.n2 * g.n3
    sums = [[0] * 7 for _ in range(bins)]
    outside = 0
    for x, y, z, vx, vy, vz in parts:
        if g.kind == FL.AMC_FIELDS_CARTESIAN:
            i = [_loop_axis(x, g.lo[0], g.hi[0], g.n1), _loop_axis(y, g.lo[1], g.hi[1], g.n2), _loop_axis(z, g.lo[2], g.hi[2], g.n3)]
            c = (vx, vy, vz)
        else:
            r = math.sqrt(x * x + y * y) if x == x and y == y else float("nan")
            i = [_loop_axis(r, g.lo[0], g.hi[0], g.n1), _loop_axis(z, g.lo[1], g.hi[1], g.n2), 0]
            c = ((x * vx + y * vy) / r, (x * vy - y * vx) / r, vz) if r > 0 else (vx, vy, vz)
        if min(i) < 0:
            outside += 1
            continue
        b = (i[0] * g.n2 + i[1]) * g.n3 + i[2]
        sums[b][0] += 1
        for k in range(3):
            sums[b][1 + k] += round(c[k] * 2.0 ** 24)        # round(): half to even
            sums[b][4 + k] += round((c[k] * c[k]) * 2.0 ** 10)
    return sums, outside


def _particles(g, rng, n):
    lo, hi = np.array(g.lo), np.array(g.hi)
    if g.kind == FL.AMC_FIELDS_CARTESIAN:
        pos = rng.uniform(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), size=(n, 3))
    else:
        r = rng.uniform(0, 1.1 * hi[0], n)
        th = rng.uniform(0, 2 * np.pi, n)
        pos = np.stack([r * np.cos(th), r * np.sin(th), rng.uniform(lo[1] - 0.1 * (hi[1] - lo[1]), hi[1] * 1.1, n)], axis=1)
    vel = rng.normal(scale=300.0, size=(n, 3))
    parts = [list(p) + list(v) for p, v in zip(pos, vel)]
    # edge cases: on the upper bound, on the axis, -0.0, NaN, exact .5 ties at 2^-24 (and 2^-10 for the squares), outside
    h = [float(v) for v in hi]
    l = [float(v) for v in lo]
    tie = 2.0 ** -25
    if g.kind == FL.AMC_FIELDS_CARTESIAN:
        parts += [[h[0], h[1], h[2], tie, 3 * tie, -tie],
                  [l[0], l[1], l[2], -3 * tie, 5 * tie, 2.0 ** -5 + 2.0 ** -30],
                  [-0.0, -0.0, -0.0, -0.0, 0.0, -0.0] if l[0] == 0 else [l[0], -0.0 if l[1] == 0 else l[1], l[2], 1.5, -2.5, 0.5],
                  [float("nan"), h[1], h[2], 1.0, 1.0, 1.0],
                  [h[0] * 2, h[1], h[2], 1.0, 1.0, 1.0],
                  [l[0] - 1e-30, l[1], l[2], 1.0, 1.0, 1.0],
                  [(l[0] + h[0]) / 2, (l[1] + h[1]) / 2, float("nan"), 2.0, 2.0, 2.0]]
    else:
        parts += [[0.0, 0.0, h[1], tie, -3 * tie, 5 * tie],              # r == 0, z == hi
                  [-0.0, -0.0, l[1], -tie, tie, 2.0 ** -5 + 2.0 ** -30],
                  [h[0], 0.0, (l[1] + h[1]) / 2, 1.0, 2.0, 3.0],              # r == hi
                  [0.0, -h[0], (l[1] + h[1]) / 2, 1.0, 2.0, 3.0],
                  [float("nan"), 0.0, h[1] / 2, 1.0, 1.0, 1.0],
                  [h[0] * 1.01, 0.0, h[1] / 2, 1.0, 1.0, 1.0],
                  [0.0, 0.0, l[1] - 1e-12, 1.0, 1.0, 1.0]]
    return parts


GRIDS = [FL.make_grid("cartesian", (3, 4, 5), (0.0, -1e-7, 2e-8), (1e-7, 1e-7, 3e-7)),
         FL.make_grid("cartesian", (1, 1, 1), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)),
         FL.make_grid("axisymmetric", (7, 9), (0.0, 0.0), (1.5e-7, 3.2e-6)),
         FL.make_grid("axisymmetric", (1, 3), (0.0, -1.0), (2.0, 1.0))]


@pytest.mark.parametrize("gi", range(len(GRIDS)))
def test_reference_equals_plain_loop(gi):
    g = GRIDS[gi]
    parts = _particles(g, np.random.default_rng(gi), 300)
    want, want_out = _loop_sample(g, parts)
    a = np.array(parts)
    got, got_out = REF.sample(g, *[a[:, k] for k in range(6)])
    assert got_out == want_out and want_out >= 3
    assert [[int(v) for v in row] for row in got] == want
    assert sum(r[0] for r in want) + want_out == len(parts)


def test_ties_round_half_to_even():
    q1, q2 = REF.quantise(np.array([2.0 ** -25, 3 * 2.0 ** -25, -(2.0 ** -25), -3 * 2.0 ** -25, 2.0 ** -5 + 2.0 ** -30]))
    assert q1.tolist() == [0, 2, 0, -2, 2 ** 19]
    assert q2.tolist()[4] == round((2.0 ** -5 + 2.0 ** -30) ** 2 * 2 ** 10)


def test_reference_rejects_out_of_range_velocity():
    g = GRIDS[1]
    x = np.full(4, 0.5)
    vx = np.array([0.0, 2.0 ** 14 - 1, 2.0 ** 14, 0.0])
    with pytest.raises(REF.RangeError) as e:
        REF.sample(g, x, x, x, vx, x, x)
    assert e.value.index == 2
    # outside the grid: not quantised, so not checked
    REF.sample(g, np.array([5.0]), np.array([0.5]), np.array([0.5]), np.array([1e9]), np.array([0.0]), np.array([0.0]))


# ---- 128-bit words ------------------------------------------------------------------------------------------------------------
def test_words_round_trip_negative_totals():
    vals = np.array([0, -1, 1, -(2 ** 63), 2 ** 63, -(2 ** 64) - 7, 2 ** 100 + 3, -(2 ** 127), 2 ** 127 - 1], dtype=object)
    w = FL.ints_to_words(vals)
    assert w[1].tolist() == [-1, -1] and w[3].tolist() == [-(2 ** 63), -1] and w[4].tolist() == [-(2 ** 63), 0]
    assert w[5].tolist() == [-7, -2]
    assert list(FL.words_to_ints(w)) == list(vals)
    # the exact sum over ranks via 32-bit limbs
    parts = [np.array([-5, 2 ** 70, -(2 ** 90)], dtype=object), np.array([3, -(2 ** 70) - 1, 2 ** 64], dtype=object)]
    limbs = sum(FL.words_to_limbs(FL.ints_to_words(p)) for p in parts)
    assert list(FL.words_to_ints(FL.limbs_to_words(limbs))) == [-2, -1, -(2 ** 90) + 2 ** 64]


# ---- derived fields ----------------------------------------------------------------------------------------------------------
def test_derived_fields_from_synthetic_totals():
    g = FL.make_grid("cartesian", (2, 1, 1), (0.0, 0.0, 0.0), (2.0, 1.0, 1.0))
    m, kb = 6.6e-26, PR.BOLTZMAN
    # bin 0: velocities (1, 0, 0) and (3, 0, 0) -> u = 2, <c^2> = 5, T_x = m/k (5 - 4); bin 1: one particle
    tot = np.zeros((2, 7), dtype=object)
    tot[0] = [2, 4 * 2 ** 24, 0, 0, 10 * 2 ** 10, 0, 0]
    tot[1] = [1, -(2 ** 23), 0, 0, 2 ** 8, 0, 0]
    f = FL.derive(g, FL.ints_to_words(tot), 4, 3, m, kb)
    assert f["count"].tolist() == [2, 1] and f["n_samples"] == 4 and f["n_outside"] == 3
    assert f["number_density"].tolist() == [2 / (4 * 1.0), 1 / (4 * 1.0)]
    assert f["velocity"][0].tolist() == [2.0, 0.0, 0.0] and f["velocity"][1, 0] == -0.5
    assert f["temperature"][0, 0] == m / kb * (5.0 - 4.0) and f["temperature"][0, 1] == 0.0
    assert f["T"][0] == (m / kb * 1.0 + 0.0 + 0.0) / 3
    assert np.isnan(f["temperature"][1]).all() and np.isnan(f["T"][1])
    assert [e.tolist() for e in f["edges"]] == [[0.0, 1.0, 2.0], [0.0, 1.0], [0.0, 1.0]]


def test_axisymmetric_volumes_sum_to_the_cylinder():
    p, _ = PR.pore_params(n=1000)
    for g in (FL.default_grid(p), FL.make_grid("axisymmetric", (5, 3), (0.0, -1.0), (2.0, 2.0))):
        v = FL.bin_volumes(g)
        assert len(v) == FL.grid_bins(g) and (v > 0).all()
        want = math.pi * g.hi[0] ** 2 * (g.hi[1] - g.lo[1])
        assert abs(v.sum() - want) <= 1e-12 * want


def test_default_grids():
    pc, _ = PR.cube_params_for_n(1000)
    g = FL.default_grid(pc)
    assert (g.kind, g.n1, g.n2, g.n3) == (FL.AMC_FIELDS_CARTESIAN, 8, 8, 8) and list(g.hi) == [pc.cube_x, pc.cube_y, pc.cube_z]
    pp, _ = PR.pore_params(n=1000)
    g = FL.default_grid(pp)
    assert (g.kind, g.n1, g.n2, g.n3) == (FL.AMC_FIELDS_AXISYMMETRIC, 16, 128, 1) and (g.hi[0], g.lo[1], g.hi[1]) == (pp.R_oa, 0.0, pp.H)
    pt, _ = PR.pore_params(n=1000, energised=True)
    assert FL.boltzmann_constant(pt) == PR.BOLTZMAN_TEMP and FL.boltzmann_constant(pp) == PR.BOLTZMAN
    a = FL.grid_to_array(FL.copy_grid(g, every=5, step_offset=7))
    h = FL.grid_from_array(a)
    assert bytes(h) == bytes(FL.copy_grid(g, every=5, step_offset=7))


# ---- the ctypes mirror of amc_field_grid ----------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("cc") is None, reason="no C compiler")
def test_field_grid_layout_matches_header(tmp_path):
    src = tmp_path / "layout.c"
    names = ["struct_size", "kind", "n1", "n2", "n3", "reserved", "every", "step_offset", "lo", "hi"]
    body = "".join(f'    printf("{k} %zu\\n", offsetof(amc_field_grid, {k}));\n' for k in names)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "argonmc.h"\nint main(void) {\n'
                   '    printf("sizeof %zu\\n", sizeof(amc_field_grid));\n' + body +
                   '    printf("max_bins %d\\n", AMC_FIELDS_MAX_BINS);\n    printf("k_fields %d %d\\n", AMC_K_FIELDS, AMC_K_COUNT);\n'
                   '    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(line.rsplit(" ", 1) for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
               if line and not line.startswith("k_fields"))
    assert int(out["sizeof"]) == C.sizeof(_abi.AmcFieldGrid)
    for k in names:
        assert int(out[k]) == getattr(_abi.AmcFieldGrid, k).offset, k
    assert int(out["max_bins"]) == _abi.AMC_FIELDS_MAX_BINS
    last = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().split("\n")[-1].split()
    assert int(last[1]) == _abi.AMC_K_NAMES.index("fields") and int(last[2]) == len(_abi.AMC_K_NAMES)


# ---- grid validation (no GPU) ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args", [("cartesian", (2049, 1, 1), (0, 0, 0), (1, 1, 1)),
                                  ("cartesian", (64, 32, 2), (0, 0, 0), (1, 1, 1)),
                                  ("cartesian", (0, 1, 1), (0, 0, 0), (1, 1, 1)),
                                  ("cartesian", (1, 1, 1), (0, 0, 1), (1, 1, 1)),
                                  ("cartesian", (1, 1, 1), (0, 0, 0), (1, float("nan"), 1)),
                                  ("axisymmetric", (4, 4, 2), (0, 0, 0), (1, 1, 1)),
                                  ("axisymmetric", (4, 4), (0.1, 0), (1, 1)),
                                  ("axisymmetric", (64, 33), (0, 0), (1, 1)),
                                  ("spherical", (1, 1, 1), (0, 0, 0), (1, 1, 1))])
def test_invalid_grids_are_refused(args):
    with pytest.raises(ValueError):
        FL.make_grid(*args)


def test_largest_grid_is_accepted():
    g = FL.make_grid("cartesian", (2048, 1, 1), (0, 0, 0), (1, 1, 1))
    assert FL.grid_bins(g) == 2048 == _abi.AMC_FIELDS_MAX_BINS
    g = FL.make_grid("axisymmetric", (16, 128, 1), (0, 0), (1, 1), every=10)
    assert (g.n3, g.every, g.struct_size) == (1, 10, C.sizeof(_abi.AmcFieldGrid))
    with pytest.raises(ValueError):
        FL.make_grid("cartesian", (1, 1, 1), (0, 0, 0), (1, 1, 1), every=-1)
