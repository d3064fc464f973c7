"""CPU only: the sampled pair distribution's host side — header, signatures and exports, the grid limits, the search box, the
derived quantities on hand-made totals, and the NumPy mirror (tests/pair_ref.py): its symmetry, its shards, a hand-counted state
and its counts in a uniform gas against the ideal-gas expectation."""
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
from argon_monte_carlo_amd import pairs as PA
from argon_monte_carlo_amd import params as PR
from tests import pair_ref as REF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["amc_pair_config", "amc_pair_sample", "amc_pair_read", "amc_pair_load", "amc_pair_reset"]
BOX = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))


def _unit(n=(1, 1, 1), r_max=0.125, **kw):
    return PA.make_grid("cartesian", n, *BOX, r_max, **kw)


# ---- header, signatures, library ------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_typed():
    main = open(os.path.join(ROOT, "include", "argonmc.h")).read()
    assert '#include "argonmc_pair.h"' in main
    assert os.path.join(ROOT, "include", "argonmc_pair.h") in _lib._source_files()
    hdr = open(os.path.join(ROOT, "include", "argonmc_pair.h")).read()
    lib = _lib.load()
    for name in NAMES:
        assert f"int {name}(amc_ctx *ctx" in hdr and hasattr(lib, name), name
    assert set(re.findall(r"^int (amc_[a-z_]+)\(", hdr, flags=re.M)) == set(_lib.PAIR_SIGNATURES) == set(NAMES)
    others = (set(_lib.SIGNATURES) | set(_lib.SHARD_SIGNATURES) | set(_lib.CORR_SIGNATURES) | set(_lib.FLUX_SIGNATURES) | set(_lib.MFP_SIGNATURES) |
              set(_lib.VDF_SIGNATURES) | set(_lib.TRANSIT_SIGNATURES))
    assert not set(NAMES) & others
    assert lib.amc_abi_version() == _abi.AMC_ABI_VERSION == 2
    assert "no error word" in hdr
    mk = open(os.path.join(ROOT, "argon_monte_carlo_amd", "csrc", "Makefile")).read()
    assert "amc_pair.o" in mk and "argonmc_pair.h" in mk


@pytest.mark.skipif(shutil.which("cc") is None, reason="no C compiler")
def test_pair_grid_layout_matches_header(tmp_path):
    src = tmp_path / "layout.c"
    names = ["struct_size", "kind", "n1", "n2", "n3", "hist_bins", "every", "step_offset", "lo", "hi", "r_max", "reserved"]
    body = "".join(f'    printf("{k} %zu\\n", offsetof(amc_pair_grid, {k}));\n' for k in names)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "argonmc.h"\nint main(void) {\n'
                   '    printf("sizeof %zu\\n", sizeof(amc_pair_grid));\n' + body +
                   '    printf("max_columns %d\\n", AMC_PAIR_MAX_COLUMNS);\n    printf("max_hist %d\\n", AMC_PAIR_MAX_HIST_BINS);\n'
                   '    printf("max_cells %d\\n", AMC_PAIR_MAX_CELLS_AXIS);\n'
                   '    printf("abi %d\\n", AMC_ABI_VERSION);\n    printf("k_count %d\\n", AMC_K_COUNT);\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(line.rsplit(" ", 1) for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n") if line)
    assert int(out["sizeof"]) == C.sizeof(_abi.AmcPairGrid) == 112
    for k in names:
        assert int(out[k]) == getattr(_abi.AmcPairGrid, k).offset, k
    assert int(out["max_columns"]) == _abi.AMC_PAIR_MAX_COLUMNS == 6144 and int(out["max_hist"]) == _abi.AMC_PAIR_MAX_HIST_BINS == 256
    assert int(out["max_cells"]) == _abi.AMC_PAIR_MAX_CELLS_AXIS == 128
    assert int(out["abi"]) == 2 and int(out["k_count"]) == len(_abi.AMC_K_NAMES) == 13      # no new kernel class


# ---- the grid limits ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [{"hist_bins": 0}, {"hist_bins": 257}, {"r_max": 0.0}, {"r_max": -1.0}, {"r_max": math.inf}, {"r_max": math.nan}])
def test_make_grid_refuses_what_the_library_would(kw):
    with pytest.raises(ValueError):
        _unit(**kw)


def test_make_grid_column_limit():
    assert PA.columns(256) == 513 and PA.columns(1) == 3 and PA.columns(64) == 129
    g = _unit((11, 1, 1), hist_bins=256)                # the most regions at the longest histogram: 5,643 columns
    assert PA.totals_shape(g) == (11, 513)
    with pytest.raises(ValueError):
        _unit((12, 1, 1), hist_bins=256)                # 6,156
    g = _unit((16, 8, 16), hist_bins=1)                 # 2,048 regions x 3 columns: the limit exactly
    assert PA.grid_bins(g) * PA.columns(g.hist_bins) == 6144 == _abi.AMC_PAIR_MAX_COLUMNS
    with pytest.raises(ValueError):
        _unit((2049, 1, 1), hist_bins=1)
    g = _unit((47, 1, 1), hist_bins=64)                 # 47 x 129 = 6,063 fit, 48 x 129 = 6,192 do not
    with pytest.raises(ValueError):
        _unit((48, 1, 1), hist_bins=64)


def test_default_grids_put_the_collision_range_on_a_column_edge():
    p, _ = PR.cube_params(n=1000)
    g = PA.default_grid(p, every=3)
    d = float(p.collision_range)
    assert (g.kind, g.n1, g.n2, g.n3, g.hist_bins, g.r_max, g.every) == (PA.AMC_FIELDS_CARTESIAN, 1, 1, 1, 64, 32.0 * d, 3)
    assert list(g.hi) == [p.cube_x, p.cube_y, p.cube_z] and PA.totals_shape(g) == (1, 129)
    assert PA.r_edges(g)[2] == d and PA.r_edges(g)[64] == g.r_max and g.r_max / 64 == d / 2
    p, _ = PR.pore_params(n=1000)
    g = PA.default_grid(p)
    assert (g.kind, g.n1, g.n2, g.n3, g.hist_bins, g.every) == (PA.AMC_FIELDS_AXISYMMETRIC, 1, 16, 1, 64, 0)
    assert (g.hi[0], g.hi[1]) == (p.R_oa, p.H) and PA.r_edges(g)[2] == float(p.collision_range)


def test_grid_array_round_trip():
    p, _ = PR.pore_params(n=1000)
    for g in (PA.default_grid(p, every=5), PA.make_grid("cartesian", (2, 3, 4), (-1.0, -2.0, 0.0), (1.0, 2.0, 3.0), 0.3, hist_bins=17, every=2, step_offset=9)):
        a = PA.grid_to_array(g)
        assert a.dtype == np.float64 and a.shape == (14,)
        assert bytes(PA.grid_from_array(a)) == bytes(g)
        h = PA.copy_grid(g, every=7, step_offset=11)
        assert (h.every, h.step_offset, h.hist_bins, h.r_max) == (7, 11, g.hist_bins, g.r_max) and type(h) is _abi.AmcPairGrid


def test_search_box_cells_and_margin():
    """The cell edge is strictly above r_max whatever the extent; one and two cells on an axis; the cap of 128."""
    g = PA.make_grid("cartesian", (1, 1, 1), (0.0, 0.0, 0.0), (0.5, 2.0, 400.0), 1.0)
    lo, hi, cells, edge = PA.search_box(g)
    assert lo == [-1.0, -1.0, -1.0] and hi == [1.5, 3.0, 401.0]
    assert cells == [2, 3, 128] and edge[2] == 402.0 / 128 and edge[0] == 1.25
    g = PA.make_grid("cartesian", (1, 1, 1), (0.0, 0.0, 0.0), (1e-9, 1e-9, 1e-9), 1.0)      # extent 2 r_max and a little: one cell
    assert PA.search_box(g)[2] == [1, 1, 1]
    g = PA.make_grid("cartesian", (1, 1, 1), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 1.0)          # 3 r_max: 2 cells (2.999997 -> floor 2)
    assert PA.search_box(g)[2] == [2, 2, 2]
    g = PA.make_grid("axisymmetric", (2, 4), (0.0, -3.0), (5.0, 7.0), 1.0)
    lo, hi, cells, edge = PA.search_box(g)
    assert lo == [-6.0, -6.0, -4.0] and hi == [6.0, 6.0, 8.0] and cells == [11, 11, 11]
    rng = np.random.RandomState(1)
    for _ in range(200):
        r_max = float(10.0 ** rng.uniform(-9, 2))
        ext = r_max * float(10.0 ** rng.uniform(-3, 3))
        g = PA.make_grid("cartesian", (1, 1, 1), (0.1, 0.2, 0.3), (0.1 + ext, 0.2 + ext, 0.3 + ext), r_max)
        _, _, cells, edge = PA.search_box(g)
        assert all(1 <= c <= 128 for c in cells) and all(e >= r_max * (1.0 + 2.0 ** -21) for e in edge)


# ---- the derived quantities ---------------------------------------------------------------------------------------------------------
def test_derive_on_hand_made_totals():
    g = PA.make_grid("cartesian", (2, 1, 1), (0.0, 0.0, 0.0), (2.0, 1.0, 1.0), 2.0, hist_bins=4)     # columns of width 0.5, regions of volume 1
    t = np.zeros((2, 9), dtype=np.int64)
    t[0] = [10, 0, 4, 6, 10, 0, 1, 6, 0]
    d = PA.derive(g, t, 5, 3, 1, 1.0)       # d = 1.0 is the edge of column 2
    assert d["r_edges"].tolist() == [0.0, 0.5, 1.0, 1.5, 2.0] and d["r_mid"].tolist() == [0.25, 0.75, 1.25, 1.75]
    vs = 4.0 * math.pi / 3.0 * np.array([0.125, 1.0 - 0.125, 3.375 - 1.0, 8.0 - 3.375])
    assert np.allclose(PA.shell_volumes(g), vs, rtol=1e-15) and np.isclose(PA.shell_volumes(g).sum(), 4.0 * math.pi / 3.0 * 8.0, rtol=1e-15)
    rho = 10 / (5 * 1.0)
    assert np.allclose(d["g"][0], np.array([0, 4, 6, 10]) / (10 * rho * vs), rtol=1e-14)
    assert np.allclose(d["g_err"][0], np.sqrt([0, 4, 6, 10]) / (10 * rho * vs), rtol=1e-14)
    assert d["coordination"][0].tolist() == [0.0, 0.4, 1.0, 2.0]
    assert d["overlap_per_centre"][0] == 0.4            # columns 0 and 1: r < 1.0
    assert np.isnan(d["approach_fraction"][0, 0]) and d["approach_fraction"][0, 1:].tolist() == [0.25, 1.0, 0.0]
    assert d["centres"].tolist() == [10, 0] and d["pairs"][0].tolist() == [0, 4, 6, 10] and d["approaching"][0].tolist() == [0, 1, 6, 0]
    # the region without centres: NaN everywhere
    assert np.isnan(d["g"][1]).all() and np.isnan(d["g_err"][1]).all() and np.isnan(d["coordination"][1]).all()
    assert np.isnan(d["overlap_per_centre"][1]) and np.isnan(d["approach_fraction"][1]).all()
    assert (d["n_samples"], d["n_outside"], d["n_unfiled"]) == (5, 3, 1) and d["shape"] == (2, 1, 1)
    # a collision range inside a column: the overlap count cannot be read off the columns
    assert np.isnan(PA.derive(g, t, 5, 3, 1, 0.75)["overlap_per_centre"]).all()
    assert PA.derive(g, t, 5, 3, 1, 1.5)["overlap_per_centre"][0] == 1.0
    # an axisymmetric grid takes the ring volumes
    ga = PA.make_grid("axisymmetric", (2, 1), (0.0, 0.0), (2.0, 3.0), 2.0, hist_bins=4)
    da = PA.derive(ga, t, 5, 0, 0, 1.0)
    assert np.allclose(da["g"][0], np.array([0, 4, 6, 10]) / (10 * (10 / (5 * math.pi * 3.0)) * vs), rtol=1e-14)


# ---- the mirror against itself ---------------------------------------------------------------------------------------------------
def _cube_state(n, seed):
    p, c = PR.cube_params_for_n(n)
    return p, c, IC.cube_ic(p, c, seed)


def test_hand_counted_state():
    """Five particles on a line, r_max = 1, H = 4: the pairs, their columns and who approaches, counted by hand."""
    g = PA.make_grid("cartesian", (1, 1, 1), (0.0, 0.0, 0.0), (10.0, 1.0, 1.0), 1.0, hist_bins=4)
    x = np.array([1.0, 1.25, 2.0, 5.0, 5.0])        # 0-1: 0.25 (column 1), 1-2: 0.75 (column 3), 0-2: 1.0 (not counted), 3-4: 0 (column 0)
    y = z = np.full(5, 0.5)
    vx = np.array([1.0, 0.0, 0.0, 2.0, 2.0])        # 0 runs into 1 (approaching); 1-2 and 3-4 at rest relative to each other
    zero = np.zeros(5)
    tot, out, unf = REF.sample(g, x, y, z, vx, zero, zero)
    want = np.zeros((1, 9), dtype=np.int64)
    want[0, 0] = 5
    want[0, 1 + 1], want[0, 1 + 3], want[0, 1 + 0] = 2, 2, 2
    want[0, 5 + 1] = 2
    assert (out, unf) == (0, 0) and np.array_equal(tot, want)
    # the index range: particle 0 alone as a centre still sees particle 1
    tot, out, unf = REF.sample(g, x, y, z, vx, zero, zero, lo=0, hi=1)
    assert tot[0].tolist() == [1, 0, 1, 0, 0, 0, 1, 0, 0]


@pytest.mark.parametrize("seed", [3, 8])
def test_single_region_columns_are_even_and_shards_add_up(seed):
    """With one region over everything every unordered pair is counted from both ends, r and s bitwise the same: even columns.
    Splitting the index range and summing reproduces the whole."""
    n = 700
    p, c, st = _cube_state(n, seed)
    st = [a.copy() for a in st]
    for a in range(3):
        st[a][5] = st[a][6]                                               # a coincident pair
    st[3][9] = math.nan                                                    # a NaN velocity: its pairs never approach
    g = PA.make_grid("cartesian", (1, 1, 1), (0, 0, 0), (p.cube_x, p.cube_y, p.cube_z), 48 * float(p.collision_range), hist_bins=12)
    tot, out, unf = REF.sample(g, *st)
    assert (out, unf) == (0, 0) and tot[0, 0] == n and tot[0, 1:].sum() > 1000 and tot[0, 1] >= 2
    assert not (tot[0, 1:] % 2).any()
    assert (tot[0, 13:] <= tot[0, 1:13]).all() and 0 < tot[0, 13:].sum() < tot[0, 1:13].sum()
    parts = [REF.sample(g, *st, lo=a, hi=b) for a, b in ((0, 1), (1, 300), (300, 301), (301, n))]
    assert np.array_equal(sum(t for t, _, _ in parts), tot) and all(u == 0 for _, _, u in parts)
    # a grid over a part of the box: the regions' centres add up to the particles inside, the rest is outside, nobody unfiled
    # but the particle moved out of the search box and the one with a NaN coordinate
    h = PA.make_grid("cartesian", (2, 1, 1), (0, 0, 0), (0.5 * p.cube_x, p.cube_y, p.cube_z), g.r_max, hist_bins=12)
    st[0][20] = p.cube_x + 1.0001 * g.r_max            # beyond the box in x (it ends at cube_x / 2 + r_max): unfiled
    st[1][21] = -1.0001 * g.r_max                       # below lo - r_max in y: unfiled
    st[2][22] = math.nan
    tot, out, unf = REF.sample(h, *st)
    assert unf == 3 and int(tot[:, 0].sum()) + out + unf == n and out > 0
    parts = [REF.sample(h, *st, lo=a, hi=b) for a, b in ((0, 233), (233, n))]
    assert np.array_equal(parts[0][0] + parts[1][0], tot) and parts[0][1] + parts[1][1] == out and parts[0][2] == parts[1][2] == unf


# ---- the definition in a uniform gas ---------------------------------------------------------------------------------------------
SEED_UNIFORM = 5


def test_uniform_gas_matches_the_ideal_gas_expectation():
    """N = 4,096 uniform in the cube at the reference density, centres in the inner box at least r_max = 32 d from every wall, H = 16
    (columns of 2 d).  A centre's shell of column k lies wholly inside the cube, the other N - 1 particles are uniform in its volume
    V, so the expected count is centres * (N - 1) / V * V_shell[k]; every column above r = d (k >= 1) must lie within five Poisson
    standard deviations sqrt(expected) of it.  Both sides are derived; the seed is fixed."""
    n = 4096
    p, c, st = _cube_state(n, SEED_UNIFORM)
    r_max = 32.0 * float(p.collision_range)
    g = PA.make_grid("cartesian", (1, 1, 1), (r_max,) * 3, (p.cube_x - r_max, p.cube_y - r_max, p.cube_z - r_max), r_max, hist_bins=16)
    tot, out, unf = REF.sample(g, *st)
    s = PA.split(g, tot)
    centres = int(s["centres"][0])
    assert unf == 0 and centres + out == n and centres > 500
    expected = centres * (n - 1) / (p.cube_x * p.cube_y * p.cube_z) * PA.shell_volumes(g)
    dev = (s["pairs"][0] - expected) / np.sqrt(expected)
    print("centres", centres, "pairs", s["pairs"][0].tolist(), "expected", np.round(expected, 1).tolist(), "deviation / sigma", np.round(dev, 2).tolist())
    assert (np.abs(dev[1:]) < 5.0).all()
    d = PA.derive(g, tot, 1, out, unf, float(p.collision_range))
    assert np.isnan(d["overlap_per_centre"]).all()      # d is the middle of column 0 here
    # velocities are independent of positions: half of the pairs approach
    frac = s["approaching"][0, 4:].sum() / s["pairs"][0, 4:].sum()
    assert abs(frac - 0.5) < 5.0 * 0.5 / math.sqrt(s["pairs"][0, 4:].sum() / 2)
