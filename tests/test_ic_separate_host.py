"""CPU only: the overlap removal of a synthetic start (include/argonmc-ic.h) — header, signatures and exports, what the call
refuses without a context, and the host mirror (tests/ic_separate_ref.py): its cell search against brute force, the rule's edges
on exact coordinates, the loop, its resume and its independence of the search cells, on the states the GPU tests use."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from argon_monte_carlo_amd import _abi, _lib
from argon_monte_carlo_amd import ic as IC
from argon_monte_carlo_amd import params as PR
from tests import ic_separate_ref as REF
from tests.philox_ref import ic_uniforms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -32                  # the crafted states' unit: min_dist = 3 U, offsets in whole U — every product and sum below is exact


def _case(kind, n, sigma_factor, seed, energised=False):
    if kind == "cube":
        p, c = PR.cube_params_for_n(n, sigma=sigma_factor * PR.SIGMA)
    else:
        p, c = PR.pore_params(n=n, sigma=sigma_factor * PR.SIGMA, energised=energised)
    return p, c, IC.device_ic_config(p, c, seed, kind), (p.cube_x, p.cube_y, p.cube_z)


@pytest.fixture(scope="module")
def cube4096():
    p, c, cfg, cube = _case("cube", 4096, 16, 12345)
    return p, cfg, cube, REF.initial_positions(cfg, cube, 4096)


@pytest.fixture(scope="module")
def cube1000():
    p, c, cfg, cube = _case("cube", 1000, 36, 7)
    return p, cfg, cube, REF.initial_positions(cfg, cube, 1000)


@pytest.fixture(scope="module")
def pore8000():
    p, c, cfg, cube = _case("pore", 8000, 100, 17)
    return p, cfg, cube, REF.initial_positions(cfg, cube, 8000)


# ---- header, signatures, library ------------------------------------------------------------------------------------------
def test_entry_point_is_declared_exported_and_typed():
    main = open(os.path.join(ROOT, "include", "argonmc.h")).read()
    assert '#include "argonmc-ic.h"' in main
    assert "amc_init_separate" not in re.sub(r"/\*.*?\*/", "", main, flags=re.S)        # declared in its own header only
    assert os.path.join(ROOT, "include", "argonmc-ic.h") in _lib._source_files()
    hdr = open(os.path.join(ROOT, "include", "argonmc-ic.h")).read()
    assert set(re.findall(r"^int (amc_[a-z_]+)\(", hdr, flags=re.M)) == set(_lib.IC_SIGNATURES) == {"amc_init_separate"}
    assert ("int amc_init_separate(amc_ctx *ctx, const amc_ic_config *cfg, double min_dist, int32_t first_round, int32_t max_rounds, "
            "int64_t *stats);") in hdr
    res, args = _lib.IC_SIGNATURES["amc_init_separate"]
    assert res is C.c_int
    assert args == [C.c_void_p, C.POINTER(_abi.AmcIcConfig), C.c_double, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]
    assert _lib.all_signatures()["amc_init_separate"] == (res, args)
    lib = _lib.load()
    assert hasattr(lib, "amc_init_separate") and lib.amc_init_separate.argtypes == args
    assert lib.amc_abi_version() == _abi.AMC_ABI_VERSION == 2
    mk = open(os.path.join(ROOT, "argon_monte_carlo_amd", "csrc", "Makefile")).read()
    hdrs = re.search(r"^HDRS = (.*)$", mk, flags=re.M).group(1).split()
    assert "../../include/argonmc-ic.h" in hdrs and "amc_cells_dev.h" in hdrs


def test_the_main_header_and_its_table_are_unchanged():
    main = open(os.path.join(ROOT, "include", "argonmc.h")).read()
    declared = set(re.findall(r"^(?:int|void|const char \*)\s*\*?\s*(amc_[a-z_]+)\s*\(", main, flags=re.M))
    assert declared == set(_lib.SIGNATURES) and "amc_init_separate" not in declared
    others = [_lib.SIGNATURES, _lib.SHARD_SIGNATURES, _lib.CORR_SIGNATURES, _lib.FLUX_SIGNATURES, _lib.MFP_SIGNATURES, _lib.VDF_SIGNATURES,
              _lib.TRANSIT_SIGNATURES, _lib.PAIR_SIGNATURES]
    assert not any("amc_init_separate" in t for t in others)
    assert len(_lib.all_signatures()) == sum(len(t) for t in others) + 1


def test_the_scan_has_one_copy():
    csrc = os.path.join(ROOT, "argon_monte_carlo_amd", "csrc")
    defs = {f: len(re.findall(r"void k_pair_scan(?:_sums)?\(", open(os.path.join(csrc, f)).read())) for f in sorted(os.listdir(csrc))
            if f.endswith((".hip", ".h"))}
    assert {f: k for f, k in defs.items() if k} == {"amc_cells_dev.h": 2}
    for f in ("amc_pair.hip", "amc_ic.hip"):
        assert '#include "amc_cells_dev.h"' in open(os.path.join(csrc, f)).read()


def test_refused_without_a_context_or_a_configuration():
    lib = _lib.load()
    p, c, cfg, cube = _case("cube", 64, 16, 1)
    st = (C.c_int64 * 8)()
    assert lib.amc_init_separate(None, C.byref(cfg), 1e-9, 1, 1, st) == -1          # AMC_ERR_INVALID
    assert lib.amc_init_separate(None, None, 1e-9, 1, 1, None) == -1


# ---- the mirror: the recipe -------------------------------------------------------------------------------------------------------
def test_round_zero_is_the_generator_and_a_round_is_another_counter():
    p, c, cfg, cube = _case("pore", 8000, 100, 17)
    for q in (0, 1, 4321, 7999):
        assert REF.uniforms(17, q, 0) == ic_uniforms(17, q)[:3]
        assert REF.uniforms(17, q, 1) != REF.uniforms(17, q, 0) and REF.uniforms(17, q, 2) != REF.uniforms(17, q, 1)
    # every region's first and last index keep to their own cylinder in every round
    for first, end, R, zl, zh in REF.regions_of(cfg):
        for q in (first, end - 1):
            for t in (0, 1, 2, 63):
                x, y, z = REF.position(cfg, cube, q, t)
                assert math.hypot(x, y) <= R * (1 + 1e-15) and zl <= z <= zh, (q, t)
    assert [REF.region_index(cfg, f) for f, *_ in REF.regions_of(cfg)] == [0, 1, 2, 3, 4]
    assert REF.region_index(cfg, 7999) == 4


# ---- the mirror: the search -------------------------------------------------------------------------------------------------------
def test_cell_search_equals_brute_force(cube1000, pore8000):
    for p, cfg, cube, (x, y, z) in (cube1000, pore8000):
        x, y, z = x[:1500], y[:1500], z[:1500]
        for md in (p.collision_range, 3 * p.collision_range):
            for cells in (1, 3, 16):
                pairs, losers = REF.search(x, y, z, md, max_cells_axis=cells)
                bp, bl = REF.brute_search(x, y, z, md)
                assert pairs == bp and np.array_equal(losers, bl)
            assert bp > 0 or md == p.collision_range


def test_the_rule_at_its_edges_on_exact_coordinates():
    md = 3 * U
    base = np.array([1000.0, 2000.0, 3000.0]) * U

    def two(off):
        a = np.array([base, base + np.array(off) * U])
        return REF.search(a[:, 0], a[:, 1], a[:, 2], md)

    for off, hit in (((2, 2, 0), True), ((2, 0, 2), True), ((0, 2, 2), True), ((2, 2, 1), False), ((1, 2, 2), False), ((3, 0, 0), False),
                     ((0, 3, 0), False), ((0, 0, 3), False), ((0, 0, 0), True), ((-2, -2, 0), True), ((-3, 0, 0), False)):
        pairs, losers = two(off)
        assert (pairs, list(losers)) == ((1, [1]) if hit else (0, [])), off
    def found(x, y, z, d=md):
        pairs, losers = REF.search(np.asarray(x, dtype=float) * U, np.asarray(y, dtype=float) * U, np.asarray(z, dtype=float) * U, d)
        return pairs, list(losers)

    # a chain i < j < k: both j and k lose, whichever of the three is in the middle unless it has the highest index
    assert found([0, 2, 4], [0, 0, 0], [0, 0, 0]) == (2, [1, 2])
    assert found([2, 0, 4], [0, 0, 0], [0, 0, 0]) == (2, [1, 2])
    assert found([0, 4, 2], [0, 0, 0], [0, 0, 0]) == (2, [2])          # the middle atom alone loses, to two partners
    # one atom over five of a lower index that keep clear of each other (12, 16 or 32 apart in squares): five pairs, one loser
    assert found([2, -2, 2, -2, 0, 0], [2, -2, -2, 2, 0, 0], [0, 0, 0, 0, 2, 0]) == (5, [5])
    assert found([0, 2, -2, 2, -2, 0], [0, 2, -2, -2, 2, 0], [0, 0, 0, 0, 0, 2]) == (5, [1, 2, 3, 4, 5])     # ... and of a higher one
    # everybody at one point
    n = 300
    pairs, losers = REF.search(np.full(n, 5 * U), np.full(n, 6 * U), np.full(n, 7 * U), md)
    assert pairs == n * (n - 1) // 2 and np.array_equal(losers, np.arange(1, n))
    assert found([1], [1], [1]) == (0, []) and found([], [], []) == (0, [])


# ---- the mirror: the loop -------------------------------------------------------------------------------------------------------
def test_cube_loop_converges_and_touches_only_losers(cube4096):
    p, cfg, cube, (x, y, z) = cube4096
    X, Y, Z, st = REF.separate(x, y, z, cfg, cube, p.collision_range)
    assert st == dict(searches=7, rounds=6, redrawn=623, pairs_first=510, losers_first=471, pairs_left=0, losers_left=0, next_round=7)
    assert REF.search(X, Y, Z, p.collision_range)[0] == 0
    _, first = REF.search(x, y, z, p.collision_range)
    moved = np.flatnonzero((X != x) | (Y != y) | (Z != z))
    assert set(first) <= set(moved) and len(moved) <= st["redrawn"]
    assert (X >= 0).all() and (X < p.cube_x).all() and (Z >= 0).all() and (Z < p.cube_z).all()
    # a query changes nothing and reports the counts
    Xq, Yq, Zq, sq = REF.separate(x, y, z, cfg, cube, p.collision_range, max_rounds=0)
    assert sq == dict(searches=1, rounds=0, redrawn=0, pairs_first=510, losers_first=471, pairs_left=510, losers_left=471, next_round=1)
    assert np.array_equal(Xq, x) and np.array_equal(Yq, y) and np.array_equal(Zq, z)


def test_a_spent_budget_resumes_where_it_stopped(cube1000):
    p, cfg, cube, (x, y, z) = cube1000
    full = REF.separate(x, y, z, cfg, cube, p.collision_range, max_rounds=64)
    assert full[3]["rounds"] == 13 and full[3]["pairs_left"] == 0
    part = REF.separate(x, y, z, cfg, cube, p.collision_range, max_rounds=3)
    assert part[3]["pairs_left"] == 82 and part[3]["next_round"] == 4 and part[3]["rounds"] == 3
    rest = REF.separate(*part[:3], cfg, cube, p.collision_range, first_round=4, max_rounds=61)
    for a, b in zip(rest[:3], full[:3]):
        assert np.array_equal(a, b)
    assert rest[3]["next_round"] == full[3]["next_round"] == 14 and rest[3]["rounds"] == 10
    assert part[3]["redrawn"] + rest[3]["redrawn"] == full[3]["redrawn"]
    assert rest[3]["pairs_first"] == part[3]["pairs_left"]


def test_pore_loop_keeps_every_atom_in_its_region(pore8000):
    p, cfg, cube, (x, y, z) = pore8000
    X, Y, Z, st = REF.separate(x, y, z, cfg, cube, p.collision_range)
    assert (st["pairs_first"], st["losers_first"], st["rounds"], st["pairs_left"]) == (218, 215, 3, 0)
    assert REF.search(X, Y, Z, p.collision_range)[0] == 0
    for first, end, R, zl, zh in REF.regions_of(cfg):
        s = slice(first, end)
        assert (np.hypot(X[s], Y[s]) <= R * (1 + 1e-15)).all() and (Z[s] >= zl).all() and (Z[s] <= zh).all()
