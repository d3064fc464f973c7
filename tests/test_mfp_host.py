"""CPU only: the sampled free paths' host side — header, signatures and exports, known answers of the quantisers and the
histogram rule (tests/mfp_ref.py against a plain Python loop), the derived quantities on random integer totals, the grid
limits, and the reference on the CPU oracle's runs of the GPU tests' scenarios."""
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
from argon_monte_carlo_amd import free_paths as FP
from argon_monte_carlo_amd import params as PR
from tests import mfp_ref as REF
from tests import mfp_states as MS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["amc_mfp_config", "amc_mfp_read", "amc_mfp_load", "amc_mfp_reset"]
UNIT = FP.make_grid("cartesian", (1, 1, 1), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), hist_bins=4, hist_hi=1e-6)
REC = _abi.path_record_dtype()


def _records(rows):
    """records from (phase, i, j, which, total, px, py, pz) rows"""
    r = np.zeros(len(rows), dtype=REC)
    for k, (phase, i, j, which, tot, px, py, pz) in enumerate(rows):
        r[k] = (0, phase, 0, i, j, which, 0, tot, px, py, pz)
    return r


def _state(n, at=0.5):
    return {"x": np.full(n, at), "y": np.full(n, at), "z": np.full(n, at)}


# ---- header, signatures, library ------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_typed():
    main = open(os.path.join(ROOT, "include", "argonmc.h")).read()
    assert '#include "argonmc_mfp.h"' in main
    assert os.path.join(ROOT, "include", "argonmc_mfp.h") in _lib._source_files()
    hdr = open(os.path.join(ROOT, "include", "argonmc_mfp.h")).read()
    lib = _lib.load()
    for name in NAMES:
        assert f"int {name}(amc_ctx *ctx" in hdr and hasattr(lib, name), name
    assert set(re.findall(r"^int (amc_[a-z_]+)\(", hdr, flags=re.M)) == set(_lib.MFP_SIGNATURES) == set(NAMES)
    assert not set(_lib.MFP_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.SHARD_SIGNATURES) | set(_lib.CORR_SIGNATURES) | set(_lib.FLUX_SIGNATURES))
    # argonmc.h itself still declares exactly SIGNATURES: the new contract is the included header's
    declared = set(re.findall(r"^(?:int|void|const char \*)\s*\*?\s*(amc_[a-z_]+)\s*\(", main, flags=re.M))
    assert declared == set(_lib.SIGNATURES) and not declared & set(NAMES)
    assert lib.amc_abi_version() == _abi.AMC_ABI_VERSION == 2
    mk = open(os.path.join(ROOT, "argon_monte_carlo_amd", "csrc", "Makefile")).read()
    assert "amc_mfp.o" in mk and "argonmc_mfp.h" in mk


@pytest.mark.skipif(shutil.which("cc") is None, reason="no C compiler")
def test_mfp_grid_layout_matches_header(tmp_path):
    src = tmp_path / "layout.c"
    names = ["struct_size", "kind", "n1", "n2", "n3", "hist_bins", "keep_records", "reserved", "lo", "hi", "hist_hi"]
    body = "".join(f'    printf("{k} %zu\\n", offsetof(amc_mfp_grid, {k}));\n' for k in names)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "argonmc.h"\nint main(void) {\n'
                   '    printf("sizeof %zu\\n", sizeof(amc_mfp_grid));\n' + body +
                   '    printf("max_columns %d\\n", AMC_MFP_MAX_COLUMNS);\n    printf("max_hist %d\\n", AMC_MFP_MAX_HIST_BINS);\n'
                   '    printf("abi %d\\n", AMC_ABI_VERSION);\n    printf("k_count %d\\n", AMC_K_COUNT);\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(line.rsplit(" ", 1) for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n") if line)
    assert int(out["sizeof"]) == C.sizeof(_abi.AmcMfpGrid) == 88
    for k in names:
        assert int(out[k]) == getattr(_abi.AmcMfpGrid, k).offset, k
    assert int(out["max_columns"]) == _abi.AMC_MFP_MAX_COLUMNS == 6144 and int(out["max_hist"]) == _abi.AMC_MFP_MAX_HIST_BINS == 64
    assert int(out["abi"]) == 2 and int(out["k_count"]) == len(_abi.AMC_K_NAMES) == 13      # no new kernel class


# ---- the quantisers -------------------------------------------------------------------------------------------------------
def _loop_record(tot, px, py, pz):
    """the six added integers of one record: Python floats, round() (half to even)"""
    return [1] + [round(math.ldexp(v, 56)) for v in (tot, px, py, pz)] + [round(math.ldexp(tot * tot, 72))]


def test_largest_values_in_range_stay_at_most_2_to_40():
    top = float(np.nextafter(2.0 ** -16, 0))
    q, q2 = REF.quantise([top, 0.0, 2.0 ** -17])
    assert [int(v) for v in q] == [round(math.ldexp(top, 56)), 0, 2 ** 39]
    # the largest double below 2^-16 is 2^-16 (1 - 2^-53): times 2^56 it lies 2^-13 below 2^40 and ROUNDS UP to it, as the fields'
    # and the fluxes' quantisers do at the top of their range — "at most 2^40", and 2^22 such records sum to at most 2^62
    assert int(q[0]) == 2 ** 40 == int(q2[0]) and int(q2[2]) == 2 ** 38
    below = float(np.nextafter(top, 0))
    assert int(REF.quantise([below * 0.999])[0][0]) < 2 ** 40
    assert _loop_record(top, top, top, top) == [1] + [int(q[0])] * 4 + [int(q2[0])]
    assert 2 ** 22 * max(int(q[0]), int(q2[0])) <= 2 ** 62 < 2 ** 63


def test_ties_round_half_to_even():
    u = 2.0 ** -57                      # half a unit of the length quantiser
    q, _ = REF.quantise([u, 3 * u, 5 * u, 7 * u, 2 * u])
    assert [int(v) for v in q] == [0, 2, 2, 4, 1]
    # the square's: total^2 2^72 = m / 2 for total = sqrt(m) 2^-36.5 — take exact squares: total = k 2^-37 gives k^2 / 4
    _, q2 = REF.quantise([k * 2.0 ** -37 for k in (1, 2, 3, 6, 10)])        # 0.25, 1, 2.25, 9, 25
    assert [int(v) for v in q2] == [0, 1, 2, 9, 25]
    _, q2 = REF.quantise([math.sqrt(2.0) * 2.0 ** -37])                      # (sqrt 2)^2 = 2.0000000000000004: 0.5000000000000001 -> 1
    assert int(q2[0]) == round(math.ldexp((math.sqrt(2.0) * 2.0 ** -37) ** 2, 72)) == 1
    t = REF.Totals(UNIT)
    t.add_step(_records([(16, 0, 1, 1, 3 * u, u, 5 * u, 7 * u)]), _state(2))
    assert [int(v) for v in t.tot[0, 1]] == [1, 2, 0, 2, 4, 0, 0]


@pytest.mark.parametrize("value", [2.0 ** -16, -1e-9, float("nan"), float("inf")])
def test_values_outside_the_range_are_reported_not_summed(value):
    rows = [(16, 5, 2, 0, 1e-7, 1e-8, 2e-8, 3e-8) for _ in range(6)]
    rows[3] = (16, 5, 4, 1, 1e-7, value, 2e-8, 3e-8)            # owner 5
    rows[1] = (3, 3, -1, 0, value, 1e-8, 2e-8, 3e-8)            # owner 3: the lowest is named
    t = REF.Totals(UNIT)
    t.add_step(_records(rows), _state(6))
    with pytest.raises(REF.RangeError) as e:
        t.check()
    assert e.value.index == 3 and t.n_records == 0 and all(int(v) == 0 for v in t.tot.ravel()) and int(t.hist.sum()) == 0
    t.add_step(_records(rows[:1]), _state(6))                   # later steps add nothing
    assert t.n_records == 0 and t.n_steps == 2
    st = _state(6)
    st["x"][[3, 5]] = 1.5                                       # outside the grid they are only counted
    t = REF.Totals(UNIT)
    t.add_step(_records(rows), st)
    t.check()
    assert (t.n_records, t.n_outside) == (4, 2) and int(t.tot[0, 1, 0]) == 4 and int(t.tot[0, 0, 0]) == 0


def test_hist_hi_lands_beyond_and_just_below_it_in_the_last_bin():
    for hb, hi in ((4, 1e-6), (32, 1e-6), (7, 3.3e-7), (64, 1e-6)):
        g = FP.make_grid("cartesian", (1, 1, 1), (0, 0, 0), (1, 1, 1), hist_bins=hb, hist_hi=hi)
        below = float(np.nextafter(hi, 0))
        cols = REF.hist_columns(g, [hi, below, 0.0, float(np.nextafter(hi, 1)), 2.0 ** -17, hi / hb, float(np.nextafter(hi / hb, 0))])
        assert cols.tolist()[:5] == [hb, hb - 1, 0, hb, hb] and cols[5] in (0, 1) and cols[6] == 0
        w = hi / hb
        for v, c in zip([below, 0.3 * hi], cols[[1]].tolist() + REF.hist_columns(g, [0.3 * hi]).tolist()):
            assert c == min(int(math.floor(v / w)), hb - 1)
    t = REF.Totals(UNIT)
    t.add_step(_records([(1, 0, -1, 0, 1e-6, 0, 0, 0), (1, 1, -1, 0, float(np.nextafter(1e-6, 0)), 0, 0, 0)]), _state(2))
    assert t.hist[0, 0].tolist() == [0, 0, 0, 1, 1] and t.hist[0, 1].tolist() == [0] * 5


def test_reference_equals_plain_loop_on_random_records():
    rng = np.random.default_rng(5)
    for g in (FP.make_grid("cartesian", (3, 2, 4), (0.0, -1e-7, 2e-8), (1e-7, 1e-7, 3e-7), hist_bins=9, hist_hi=4e-7),
              FP.make_grid("axisymmetric", (2, 9), (0.0, 0.0), (1.5e-7, 3.2e-6), hist_bins=0)):
        n, m = 50, 400
        lo, hi = np.array(g.lo), np.array(g.hi)
        if g.kind == FP.AMC_FIELDS_CARTESIAN:
            pos = rng.uniform(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), size=(n, 3))
        else:
            r, th = rng.uniform(0, 1.1 * hi[0], n), rng.uniform(0, 2 * np.pi, n)
            pos = np.stack([r * np.cos(th), r * np.sin(th), rng.uniform(-0.1 * hi[1], 1.1 * hi[1], n)], axis=1)
        st = {"x": pos[:, 0].copy(), "y": pos[:, 1].copy(), "z": pos[:, 2].copy()}
        rows = []
        for _ in range(m):
            i, j = rng.choice(n, 2, replace=False)
            v = rng.exponential(8e-8, 4)
            if rng.random() < 0.4:
                rows.append((int(rng.integers(1, 16)), int(i), -1, 0, *v))
            else:
                rows.append((16 + int(rng.integers(0, 8)), int(max(i, j)), int(min(i, j)), int(rng.integers(0, 2)), *v))
        rec = _records(rows)
        t = REF.Totals(g)
        t.add_step(rec[:150], st)
        t.add_step(rec[150:], st)
        t.check()
        bins, hb = FP.grid_bins(g), int(g.hist_bins)
        want = [[[0] * 7 for _ in range(2)] for _ in range(bins)]
        wh = [[[0] * (hb + 1) for _ in range(2)] for _ in range(bins)]
        outside = 0
        pb = REF.position_bins(g, st["x"], st["y"], st["z"])
        for phase, i, j, which, tot, px, py, pz in rows:
            kind = 1 if phase >= 16 else 0
            owner = (i if which else j) if kind else i
            if pb[owner] < 0:
                outside += 1
                continue
            cell = want[pb[owner]][kind]
            for q, v in enumerate(_loop_record(tot, px, py, pz)):
                cell[q] += v
            if hb:
                wh[pb[owner]][kind][min(int(math.floor(tot / (g.hist_hi / hb))), hb - 1) if tot < g.hist_hi else hb] += 1
        assert outside == t.n_outside >= 3 and t.n_records == m - outside and t.n_steps == 2
        assert [[[int(v) for v in k] for k in b] for b in t.tot] == want and t.hist.tolist() == wh
        assert all(int(v) == 0 for v in t.tot[:, :, 6].ravel())          # the reserved word is never added to


# ---- derive ---------------------------------------------------------------------------------------------------------------
def test_derive_equals_fraction_arithmetic_on_random_integer_totals():
    g = FP.make_grid("axisymmetric", (3, 4), (0.0, 0.0), (1.5e-7, 3.2e-6), hist_bins=5, hist_hi=1e-6)
    rng = np.random.default_rng(11)
    sums = np.zeros((12, 2, 7), dtype=object)
    hist = np.zeros((12, 2, 6), dtype=np.int64)
    for b in range(12):
        for k in range(2):
            n = 0 if (b + k) % 5 == 0 else int(rng.integers(1, 10 ** 6)) * (10 ** 12 if b == 11 else 1)      # (bin 11: beyond 64 bits)
            if b == 3:
                n = 0
            m = float(rng.uniform(2e-8, 2e-7))
            sums[b, k] = [n] + [int(n * m * f * 2 ** 56 + rng.integers(-2 ** 20, 2 ** 20)) * (n > 0) for f in (1, 0.5, 0.4, 0.6)] + \
                         [int(n * 2 * m * m * 2 ** 72) * (n > 0), 0]
            if n and b != 7:
                hist[b, k] = rng.multinomial(min(n, 10 ** 9), [0.3, 0.25, 0.2, 0.1, 0.1, 0.05])
    assert max(abs(int(v)) for v in sums.ravel()) > 2 ** 64
    f = FP.derive(g, FP.ints_to_words(sums), hist, 100, 3, 7, 2.5e-12)
    want = REF.derive(g, sums, hist, 7, 2.5e-12)
    for k, w in want.items():
        if k in REF.INEXACT:        # (float arithmetic in the product, an exact rational rounded once in the reference)
            assert np.allclose(f[k], w, rtol=2.0 ** -51, atol=0.0, equal_nan=True) and np.array_equal(np.isnan(f[k]), np.isnan(w)), k
        else:
            assert np.array_equal(f[k], w, equal_nan=True), k
    # by hand, one entry: the mean and the wall's share
    n0, n1 = int(sums[5, 0, 0]), int(sums[5, 1, 0])
    assert f["mean_free_path"][5, 2] == float(Fraction(int(sums[5, 0, 1]) + int(sums[5, 1, 1]), (n0 + n1) * 2 ** 56))
    assert f["wall_fraction"][5] == float(Fraction(n0, n0 + n1)) and f["count"][5].tolist() == [n0, n1, n0 + n1]
    assert f["end_rate"][5, 1] == n1 / (7 * 2.5e-12 * f["bin_volume"][5])
    # empty (bin, kind)s give NaN, not a warning; an empty bin a NaN wall fraction and rate 0
    assert np.isnan(f["mean_free_path"][3]).all() and np.isnan(f["wall_fraction"][3]) and (f["end_rate"][3] == 0.0).all()
    assert np.isnan(f["var_free_path"][0, 0]) and np.isfinite(f["var_free_path"][0, 1]) and np.isnan(f["hist_density"][7]).all()
    d = f["hist_density"][5, 2]
    assert np.allclose(d.sum() * (1e-6 / 5), 1.0, rtol=1e-14) and np.array_equal(d, (hist[5, 0, :5] + hist[5, 1, :5]) / (hist[5, :, :5].sum()) / (1e-6 / 5))
    assert f["hist"].shape == (12, 3, 6) and f["hist_edges"].tolist() == np.linspace(0, 1e-6, 6).tolist()
    assert (f["n_records"], f["n_outside"], f["n_steps"], f["shape"], f["totals"].shape) == (100, 3, 7, (3, 4, 1), (12, 2, 7, 2))
    assert np.isnan(FP.derive(g, FP.ints_to_words(sums), hist, 0, 0, 0, 2.5e-12)["end_rate"]).all()


# ---- grids ------------------------------------------------------------------------------------------------------------------
def test_6144_columns_are_accepted_and_one_more_refused():
    g = FP.make_grid("cartesian", (8, 8, 6), (0, 0, 0), (1, 1, 1), hist_bins=0)            # 384 x 2 x 8
    assert FP.columns(FP.grid_bins(g), 0) == 6144 == _abi.AMC_MFP_MAX_COLUMNS
    assert FP.columns(FP.grid_bins(FP.make_grid("cartesian", (4, 4, 4), (0, 0, 0), (1, 1, 1), hist_bins=40)), 40) == 6144
    assert FP.columns(FP.grid_bins(FP.make_grid("axisymmetric", (4, 12), (0, 0), (1, 1), hist_bins=56)), 56) == 6144
    for n, hb in [((8, 8, 6), 1), ((385, 1, 1), 0), ((4, 4, 4), 41), ((43, 1, 1), 64)]:
        assert FP.columns(n[0] * n[1] * n[2], hb) > 6144
        with pytest.raises(ValueError):
            FP.make_grid("cartesian", n, (0, 0, 0), (1, 1, 1), hist_bins=hb)
    assert FP.columns(42, 64) == 6048
    FP.make_grid("cartesian", (42, 1, 1), (0, 0, 0), (1, 1, 1), hist_bins=64)
    for bad in (dict(hist_bins=65), dict(hist_bins=-1), dict(hist_hi=0.0), dict(hist_hi=float("inf")), dict(hist_hi=float("nan"))):
        with pytest.raises(ValueError):
            FP.make_grid("cartesian", (1, 1, 1), (0, 0, 0), (1, 1, 1), **bad)
    assert isinstance(g, _abi.AmcMfpGrid) and (g.struct_size, g.keep_records, g.reserved) == (C.sizeof(_abi.AmcMfpGrid), 0, 0)
    h = FP.copy_grid(g, keep_records=True)
    assert (h.keep_records, g.keep_records) == (1, 0) and FP.totals_shape(g) == (384, 2, 7, 2) and FP.hist_shape(g) == (384, 2, 1)


def test_default_grids_and_checkpoint_arrays():
    pc, _ = PR.cube_params_for_n(1000)
    g = FP.default_grid(pc)
    assert (g.kind, g.n1, g.n2, g.n3, g.hist_bins, g.hist_hi, g.keep_records) == (FP.AMC_FIELDS_CARTESIAN, 4, 4, 4, 32, 1e-6, 0)
    assert list(g.lo) == [0.0, 0.0, 0.0] and list(g.hi) == [pc.cube_x, pc.cube_y, pc.cube_z]
    assert FP.columns(64, 32) == 5120 <= 6144
    for energised in (False, True):
        pp, _ = PR.pore_params(n=1000, energised=energised)
        g = FP.default_grid(pp, keep_records=True)
        assert (g.kind, g.n1, g.n2, g.n3, g.hist_bins, g.hist_hi, g.keep_records) == (FP.AMC_FIELDS_AXISYMMETRIC, 4, 16, 1, 32, 1e-6, 1)
        assert (g.lo[0], g.hi[0], g.lo[1], g.hi[1]) == (0.0, pp.R_oa, 0.0, pp.H)
        h = FP.grid_from_array(FP.grid_to_array(g))
        assert isinstance(h, _abi.AmcMfpGrid) and bytes(h) == bytes(g)
    g = FP.make_grid("cartesian", (3, 2, 4), (0.0, -1e-7, 2e-8), (1e-7, 1e-7, 3e-7), hist_bins=9, hist_hi=4e-7)
    assert bytes(FP.grid_from_array(FP.grid_to_array(g))) == bytes(g)
    assert len(FP.QUANTITIES) == 7 and FP.QUANTITIES[0] == "count" and FP.QUANTITIES[6] == "reserved"
    w = FP.ints_to_words(np.array([[-(2 ** 100), 2 ** 70 + 5]], dtype=object))
    assert [int(v) for v in FP.words_to_ints(w).ravel()] == [-(2 ** 100), 2 ** 70 + 5]


# ---- the scenarios of the GPU tests, on the CPU oracle --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_reference_conserves_the_oracles_events(name):
    p, _, _ = MS.scenario_params(name)
    steps = MS.oracle_steps(name)
    t = REF.Totals(FP.default_grid(p))
    wall = pp = 0
    for k, (rec, st) in enumerate(steps):
        ww, cc = MS.ORACLE_COUNTS[name][k]
        kinds = REF.owners_and_kinds(rec)[1]
        assert int(kinds.sum()) == cc and (ww is None or int((kinds == 0).sum()) == ww)
        wall += int((kinds == 0).sum())
        pp += int(kinds.sum())
        before = (t.n_records, t.n_outside)
        t.add_step(rec, st)
        assert t.n_records + t.n_outside - sum(before) == len(rec)
    t.check()
    # per kind: the bins' counts plus the owners outside are the oracle's records (an owner outside is of either kind)
    counts = [sum(int(v) for v in t.tot[:, k, 0]) for k in range(2)]
    assert counts[0] <= wall and counts[1] <= pp and counts[0] + counts[1] + t.n_outside == wall + pp
    if t.n_outside == 0:
        assert counts == [wall, pp]
    assert int(t.hist.sum()) == t.n_records and t.n_steps == MS.STEPS[name]
    if name == "B":
        assert wall > 0 and pp > 0
    if name == "A":
        assert all(c > 0 for _, c in MS.ORACLE_COUNTS["A"]) and wall == 0
    if name == "C":
        owner = REF.owners_and_kinds(steps[0][0])[0]
        assert len(owner) == 3024 > 2048 and len(owner) - len(np.unique(owner)) == 267
