"""CPU only: the sampled correlations' host side — the NumPy reference (tests/corr_ref.py) against a plain Python loop, the
derived quantities on constructed totals, the 128-bit words, the grid validation and the ctypes mirror of amc_corr_grid."""
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
from argon_monte_carlo_amd import correlations as CO
from argon_monte_carlo_amd import params as PR
from tests import corr_ref as REF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


# ---- the reference against a plain per-particle loop ------------------------------------------------------------------------
def _loop_axis(u, lo, hi, n):
    w = (hi - lo) / n
    v = (u - lo) / w
    if v != v:
        return -1
    i = math.floor(v)
    if i == n and u <= hi:
        return n - 1
    return i if 0 <= i < n else -1


def _loop_group(g, x, y, z):
    if g.kind == CO.AMC_FIELDS_CARTESIAN:
        i = [_loop_axis(x, g.lo[0], g.hi[0], g.n1), _loop_axis(y, g.lo[1], g.hi[1], g.n2), _loop_axis(z, g.lo[2], g.hi[2], g.n3)]
    else:
        r = math.sqrt(x * x + y * y) if x == x and y == y else NAN
        i = [_loop_axis(r, g.lo[0], g.hi[0], g.n1), _loop_axis(z, g.lo[1], g.hi[1], g.n2), 0]
    return -1 if min(i) < 0 else (i[0] * g.n2 + i[1]) * g.n3 + i[2]


def _loop_sample(g, origin, current):
    """(sums[groups][7], outside, lowest index out of range or None): one particle after the other, Python floats and ints."""
    sums = [[0] * 7 for _ in range(CO.grid_groups(g))]
    outside, bad = 0, None
    for p, (o, c) in enumerate(zip(origin, current)):
        b = _loop_group(g, o[0], o[1], o[2])
        if b < 0:
            outside += 1
            continue
        d = [c[k] - o[k] for k in range(3)]
        if not (all(abs(v) < 2.0 ** -18 for v in d) and all(abs(v) < 2.0 ** 14 for v in c[3:]) and all(abs(v) < 2.0 ** 14 for v in o[3:])):
            bad = p if bad is None else bad
            continue
        sums[b][0] += 1
        for k in range(3):
            sums[b][1 + k] += round(math.ldexp(d[k] * d[k], 74))        # round(): half to even
            sums[b][4 + k] += round((c[3 + k] * o[3 + k]) * 2.0 ** 10)
    return sums, outside, bad


def _random_pair(g, rng, n):
    lo, hi = np.array(g.lo), np.array(g.hi)
    if g.kind == CO.AMC_FIELDS_CARTESIAN:
        pos = rng.uniform(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), size=(n, 3))
    else:
        r = rng.uniform(0, 1.1 * hi[0], n)
        th = rng.uniform(0, 2 * np.pi, n)
        pos = np.stack([r * np.cos(th), r * np.sin(th), rng.uniform(lo[1] - 0.1 * (hi[1] - lo[1]), hi[1] * 1.1, n)], axis=1)
    origin = np.concatenate([pos, rng.normal(scale=300.0, size=(n, 3))], axis=1)
    move = rng.normal(scale=2e-8, size=(n, 3)) * rng.choice([1.0, 1e-3, 30.0], size=(n, 1))
    current = np.concatenate([pos + move, rng.normal(scale=300.0, size=(n, 3))], axis=1)
    return origin, current


GRIDS = [CO.make_grid("cartesian", (3, 2, 4), (0.0, -1e-7, 2e-8), (1e-7, 1e-7, 3e-7), n_lags=2),
         CO.make_grid("cartesian", (1, 1, 1), (0.0, 0.0, 0.0), (1e-6, 1e-6, 1e-6), n_lags=1),
         CO.make_grid("axisymmetric", (2, 9), (0.0, 0.0), (1.5e-7, 3.2e-6), n_lags=3),
         CO.make_grid("axisymmetric", (1, 32), (0.0, 0.0), (1.5e-7, 3.2e-6), n_lags=16)]


@pytest.mark.parametrize("gi", range(len(GRIDS)))
def test_reference_equals_plain_loop_on_random_states(gi):
    g = GRIDS[gi]
    origin, current = _random_pair(g, np.random.default_rng(gi), 400)
    want, want_out, bad = _loop_sample(g, origin.tolist(), current.tolist())
    assert bad is None and want_out >= 3
    got, got_out = REF.sample(g, origin.T, current.T)
    assert got_out == want_out
    assert [[int(v) for v in row] for row in got] == want
    assert sum(r[0] for r in want) + want_out == 400
    assert any(r[1] for r in want) and any(r[4] for r in want)


def _edge_case(g):
    """origin / current rows at the exact edges of the bin rule and of the quantisers' range, all in a one-group box."""
    h, l = [float(v) for v in g.hi], [float(v) for v in g.lo]
    mid = [(a + b) / 2 for a, b in zip(l, h)]
    tie = 2.0 ** -37                        # (tie * tie) * 2^74 = 1
    rows = [
        (h + [1.0, 2.0, 3.0], h + [1.0, 2.0, 3.0]),                                             # u == hi: the last bin
        ([np.nextafter(h[0], math.inf), mid[1], mid[2], 1.0, 1.0, 1.0], mid + [1.0, 1.0, 1.0]),  # just beyond hi: outside
        ([NAN, mid[1], mid[2], 1.0, 1.0, 1.0], mid + [1.0, 1.0, 1.0]),                          # NaN origin: outside
        ([mid[0], mid[1], NAN, 2.0 ** 20, 1.0, 1.0], mid + [NAN, 1.0, 1.0]),                    # outside: not examined at all
        (mid + [3.0, -4.0, 5.0], [mid[0] + tie, mid[1] - 3 * tie, mid[2], -0.5, 2.0 ** -11, 2.0 ** -12]),
        ([0.0, mid[1], mid[2], 2.0 ** 14 - 1.0, 1.0, 1.0], [np.nextafter(2.0 ** -18, 0), mid[1], mid[2], -(2.0 ** 14 - 1.0), 1.0, 1.0]),  # the largest in range
        (l + [0.0, -0.0, 1.0], l + [1.0, 1.0, 3 * 2.0 ** -11]),                                 # c_z = rint(1.5): a tie -> 2
    ]
    return [r[0] for r in rows], [r[1] for r in rows]


def test_reference_equals_plain_loop_at_the_edges():
    g = CO.make_grid("cartesian", (1, 1, 1), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), n_lags=1)
    origin, current = _edge_case(g)
    want, want_out, bad = _loop_sample(g, origin, current)
    assert bad is None and want_out == 3
    got, got_out = REF.sample(g, np.array(origin).T, np.array(current).T)
    assert got_out == 3 and [[int(v) for v in row] for row in got] == want
    assert want[0][0] == 4
    # the largest values in range: at most 2^38 in magnitude (the square of the largest displacement rounds up to it)
    assert REF.quantise_c([2.0 ** 14 - 1.0], [-(2.0 ** 14 - 1.0)])[0] == -((2 ** 14 - 1) ** 2) * 2 ** 10
    assert REF.quantise_m([np.nextafter(2.0 ** -18, 0)])[0] == 2 ** 38
    # ties round half to even
    assert REF.quantise_c([1.0, 3.0, 5.0, -3.0], [2.0 ** -11] * 4) == [0, 2, 2, -2]
    assert REF.quantise_m([2.0 ** -37, 3 * 2.0 ** -37, -(2.0 ** -18) / 2]) == [1, 9, 2 ** 36]


@pytest.mark.parametrize("which,value", [("d", 2.0 ** -18), ("d", -(2.0 ** -18)), ("v", 2.0 ** 14), ("v", -(2.0 ** 14)),
                                         ("v0", 2.0 ** 14), ("v", NAN), ("d", NAN)])
def test_values_on_the_range_limits_are_reported_not_summed(which, value):
    g = CO.make_grid("cartesian", (1, 1, 1), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), n_lags=1)
    n = 6
    origin = np.tile(np.array([0.5, 0.5, 0.5, 10.0, 20.0, 30.0]), (n, 1))
    current = origin.copy()
    current[:, 0] += 2.0 ** -20
    for p in (4, 2):                    # two offenders: the lowest index is named
        if which == "d":
            current[p, 1] = origin[p, 1] + value        # (0.5 + 2^-18 is exact)
        elif which == "v":
            current[p, 5] = value
        else:
            origin[p, 4] = value
    with pytest.raises(REF.RangeError) as e:
        REF.sample(g, origin.T, current.T)
    assert e.value.index == 2
    assert _loop_sample(g, origin.tolist(), current.tolist())[2] == 2
    # the same offenders with their origin outside the grid take no part: nothing to report
    origin[[2, 4], 0] = 1.5
    got, out = REF.sample(g, origin.T, current.T)
    assert out == 2 and int(got[0, 0]) == n - 2


def test_window_turns_over_at_n_lags():
    g = CO.make_grid("cartesian", (1, 1, 1), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), n_lags=2)
    rng = np.random.default_rng(1)
    base = np.concatenate([rng.uniform(0.2, 0.8, size=(3, 50)), rng.normal(scale=100.0, size=(3, 50))])
    states = [tuple(base + np.concatenate([np.full((3, 50), k * 1e-8), np.zeros((3, 50))])) for k in range(6)]
    w = REF.Window(g)
    pos = []
    for s in states:
        w.add(s)
        pos.append(w.pos)
    assert pos == [1, 2, 1, 2, 1, 2]        # origin, lag 1, lag 2 + origin, lag 1, lag 2 + origin, lag 1
    assert w.counters() == (3, 6, 0, 2)
    assert [int(w.totals[0, l, 0]) for l in range(3)] == [150, 150, 100]
    # lag l moved every particle by l * 1e-8 along each axis
    pairs = {1: [(0, 1), (2, 3), (4, 5)], 2: [(0, 2), (2, 4)]}
    for l in (1, 2):
        want = sum(sum(REF.quantise_m(states[b][0] - states[a][0])) for a, b in pairs[l])
        assert int(w.totals[0, l, 1]) == want > 0
        want_c = sum(sum(REF.quantise_c(states[b][3], states[a][3])) for a, b in pairs[l])
        assert int(w.totals[0, l, 4]) == want_c


# ---- derived quantities ---------------------------------------------------------------------------------------------------
def test_derive_geometric_vacf_has_the_known_trapezoid_sum():
    g = CO.make_grid("cartesian", (2, 1, 1), (0.0, 0.0, 0.0), (2.0, 1.0, 1.0), n_lags=4)
    tot = np.empty((2, 5, 7), dtype=object)
    tot[:] = 0
    cnt, c0, dt, every = 1000, 90000, 2.5e-13, 4
    for l in range(5):
        # group 0: vacf = c0 / 2^l (exact in binary); msd_x grows like (l * 3e-9)^2
        tot[0, l] = [cnt, l * l * 9 * 2 ** 20 * cnt, 0, 0, (c0 * 2 ** 10 * cnt) >> l, 0, -(c0 * 2 ** 10 * cnt) >> l]
    f = CO.derive(g, CO.ints_to_words(tot), (3, 12, 7, 2), dt, every)
    assert f["count"].tolist() == [[cnt] * 5, [0] * 5]
    assert (f["n_origins"], f["n_samples"], f["n_outside"], f["window_pos"]) == (3, 12, 7, 2)
    assert f["lag_time"].tolist() == [l * (every * dt) for l in range(5)]
    vac = [Fraction(c0, 2 ** l) for l in range(5)]
    assert [Fraction(v) for v in f["vacf"][0, :, 0]] == vac and [Fraction(v) for v in f["vacf"][0, :, 2]] == [-v for v in vac]
    trap = sum((vac[l] + vac[l + 1]) / 2 for l in range(4))
    assert trap == Fraction(c0) * (Fraction(1, 2) + Fraction(1, 2) + Fraction(1, 4) + Fraction(1, 8) + Fraction(1, 32))
    assert f["D_vacf"][0, 0] == float(trap) * (every * dt) and f["D_vacf"][0, 2] == -f["D_vacf"][0, 0] and f["D_vacf"][0, 1] == 0.0
    for l in range(5):
        want = Fraction(l * l * 9 * 2 ** 20, 2 ** 74)
        assert Fraction(f["msd"][0, l, 0]) == Fraction(float(want))
        if l:
            assert f["D_msd"][0, l, 0] == float(want) / (2 * (l * (every * dt)))
    assert np.isnan(f["D_msd"][0, 0]).all()
    assert np.isnan(f["msd"][1]).all() and np.isnan(f["D_vacf"][1]).all()


def test_derive_uses_each_lags_own_count_in_an_incomplete_window():
    g = CO.make_grid("cartesian", (1, 1, 1), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), n_lags=3)
    tot = np.empty((1, 4, 7), dtype=object)
    tot[:] = 0
    # two origins, the second window stopped after lag 1: counts 200, 200, 100, 100; lag 3 of a third run never reached
    tot[0, 0] = [200, 0, 0, 0, 200 * 7 * 2 ** 10, 0, 0]
    tot[0, 1] = [200, 200 * 2 ** 30, 0, 0, 200 * 5 * 2 ** 10, 0, 0]
    tot[0, 2] = [100, 100 * 2 ** 32, 0, 0, 100 * 3 * 2 ** 10, 0, 0]
    tot[0, 3] = [0, 0, 0, 0, 0, 0, 0]
    f = CO.derive(g, CO.ints_to_words(tot), (2, 5, 0, 2), 1e-12, 1)
    assert f["count"][0].tolist() == [200, 200, 100, 0]
    assert f["vacf"][0, :3, 0].tolist() == [7.0, 5.0, 3.0] and np.isnan(f["vacf"][0, 3, 0])
    assert f["msd"][0, 1, 0] == 2.0 ** -44 and f["msd"][0, 2, 0] == 2.0 ** -42
    assert f["D_vacf"][0, 0] == (6.0 + 4.0) * 1e-12         # the trapezoid over the lags that have a count


# ---- 128-bit words -------------------------------------------------------------------------------------------------------
def test_words_and_limbs_round_trip_negative_sums():
    vals = np.array([[0, -1, 2 ** 62], [-(2 ** 62) * 5, -(2 ** 100) - 9, 2 ** 127 - 1]], dtype=object)
    w = CO.ints_to_words(vals)
    assert w.shape == (2, 3, 2) and w[0, 1].tolist() == [-1, -1]
    assert CO.words_to_ints(w).tolist() == vals.tolist()
    parts = [np.array([-(2 ** 62), 2 ** 70, -3], dtype=object), np.array([-(2 ** 62), -(2 ** 70) - 1, 5], dtype=object)]
    limbs = sum(CO.words_to_limbs(CO.ints_to_words(p)) for p in parts)
    assert list(CO.words_to_ints(CO.limbs_to_words(limbs))) == [-(2 ** 63), -1, 2]


# ---- grids ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args,kw", [(("cartesian", (257, 1, 1), (0, 0, 0), (1, 1, 1)), {}),
                                     (("cartesian", (8, 8, 5), (0, 0, 0), (1, 1, 1)), {}),
                                     (("cartesian", (0, 1, 1), (0, 0, 0), (1, 1, 1)), {}),
                                     (("cartesian", (1, 1, 1), (0, 0, 1), (1, 1, 1)), {}),
                                     (("cartesian", (1, 1, 1), (0, 0, 0), (1, NAN, 1)), {}),
                                     (("axisymmetric", (4, 4, 2), (0, 0, 0), (1, 1, 1)), {}),
                                     (("axisymmetric", (4, 4), (0.1, 0), (1, 1)), {}),
                                     (("spherical", (1, 1, 1), (0, 0, 0), (1, 1, 1)), {}),
                                     (("cartesian", (1, 1, 1), (0, 0, 0), (1, 1, 1)), {"n_lags": 0}),
                                     (("cartesian", (1, 1, 1), (0, 0, 0), (1, 1, 1)), {"n_lags": 65536}),
                                     (("cartesian", (256, 1, 1), (0, 0, 0), (1, 1, 1)), {"n_lags": 256}),
                                     (("cartesian", (1, 1, 1), (0, 0, 0), (1, 1, 1)), {"every": -1}),
                                     (("cartesian", (1, 1, 1), (0, 0, 0), (1, 1, 1)), {"step_offset": -1})])
def test_invalid_grids_are_refused(args, kw):
    with pytest.raises(ValueError):
        CO.make_grid(*args, **kw)


def test_largest_grids_are_accepted_and_copies_are_checked():
    g = CO.make_grid("cartesian", (256, 1, 1), (0, 0, 0), (1, 1, 1), n_lags=255)
    assert CO.grid_groups(g) == 256 == _abi.AMC_CORR_MAX_GROUPS and CO.totals_shape(g) == (256, 256, 7, 2)
    assert 256 * 256 == _abi.AMC_CORR_MAX_CELLS
    g = CO.make_grid("cartesian", (1, 1, 1), (0, 0, 0), (1, 1, 1), n_lags=65535, every=10)
    assert (g.n_lags, g.every, g.struct_size, list(g.reserved)) == (65535, 10, C.sizeof(_abi.AmcCorrGrid), [0, 0])
    h = CO.copy_grid(g, every=3, step_offset=7, n_lags=2)
    assert (h.every, h.step_offset, h.n_lags, g.n_lags) == (3, 7, 2, 65535)
    with pytest.raises(ValueError):
        CO.copy_grid(g, n_lags=65536)
    with pytest.raises(ValueError):
        CO.copy_grid(g, every=-2)


def test_default_grids_and_checkpoint_arrays():
    pc, _ = PR.cube_params_for_n(1000)
    g = CO.default_grid(pc)
    assert (g.kind, g.n1, g.n2, g.n3) == (CO.AMC_FIELDS_CARTESIAN, 1, 1, 1) and list(g.lo) == [0.0, 0.0, 0.0]
    assert list(g.hi) == [pc.cube_x, pc.cube_y, pc.cube_z] and g.n_lags == CO.DEFAULT_N_LAGS and g.every == 0
    for energised in (False, True):
        pp, _ = PR.pore_params(n=1000, energised=energised)
        g = CO.default_grid(pp, every=5, n_lags=8)
        assert (g.kind, g.n1, g.n2, g.n3, g.n_lags, g.every) == (CO.AMC_FIELDS_AXISYMMETRIC, 1, 32, 1, 8, 5)
        assert (g.lo[0], g.hi[0], g.lo[1], g.hi[1]) == (0.0, pp.R_oa, 0.0, pp.H)
    h = CO.grid_from_array(CO.grid_to_array(CO.copy_grid(g, step_offset=9)))
    assert bytes(h) == bytes(CO.copy_grid(g, step_offset=9))


# ---- the ctypes mirror and the exports --------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("cc") is None, reason="no C compiler")
def test_corr_grid_layout_matches_header(tmp_path):
    src = tmp_path / "layout.c"
    names = ["struct_size", "kind", "n1", "n2", "n3", "n_lags", "every", "step_offset", "lo", "hi", "reserved"]
    body = "".join(f'    printf("{k} %zu\\n", offsetof(amc_corr_grid, {k}));\n' for k in names)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "argonmc.h"\nint main(void) {\n'
                   '    printf("sizeof %zu\\n", sizeof(amc_corr_grid));\n' + body +
                   '    printf("max_groups %d\\n", AMC_CORR_MAX_GROUPS);\n    printf("max_cells %d\\n", AMC_CORR_MAX_CELLS);\n'
                   '    printf("abi %d\\n", AMC_ABI_VERSION);\n    printf("k_count %d\\n", AMC_K_COUNT);\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(line.rsplit(" ", 1) for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n") if line)
    assert int(out["sizeof"]) == C.sizeof(_abi.AmcCorrGrid)
    for k in names:
        assert int(out[k]) == getattr(_abi.AmcCorrGrid, k).offset, k
    assert int(out["max_groups"]) == _abi.AMC_CORR_MAX_GROUPS and int(out["max_cells"]) == _abi.AMC_CORR_MAX_CELLS
    assert int(out["abi"]) == 2 and int(out["k_count"]) == len(_abi.AMC_K_NAMES) == 13


def test_entry_points_are_declared_exported_and_typed():
    assert '#include "argonmc_corr.h"' in open(os.path.join(ROOT, "include", "argonmc.h")).read()
    assert os.path.join(ROOT, "include", "argonmc_corr.h") in _lib._source_files()
    hdr = open(os.path.join(ROOT, "include", "argonmc_corr.h")).read()
    names = ["amc_corr_config", "amc_corr_sample", "amc_corr_read", "amc_corr_origin", "amc_corr_load", "amc_corr_reset"]
    lib = _lib.load()
    for name in names:
        assert f"int {name}(amc_ctx *ctx" in hdr and name in _lib.CORR_SIGNATURES and hasattr(lib, name), name
    assert set(re.findall(r"^int (amc_[a-z_]+)\(", hdr, flags=re.M)) == set(_lib.CORR_SIGNATURES) == set(names)
    assert not set(_lib.CORR_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.SHARD_SIGNATURES))
    assert "sampled correlations" in hdr and "amc_corr_reset" in hdr.split("None of these restarts a window")[1][:200]
    mk = open(os.path.join(ROOT, "argon_monte_carlo_amd", "csrc", "Makefile")).read()
    assert "amc_corr.o" in mk
