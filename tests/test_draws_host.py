"""Host (no GPU): the references that tests/test_gpu_draws.py holds the device draws against (tests/draw_ref.py), the
crafted state they are drawn on (edge_states.temp_draw_hits()) and the table of chosen draws.

The table: tools/find_draws.py searched the draws of SEED over steps in [0, 2^30) and the state's plane-case particles
(normals (0, 0, +-1): the outcome is known before any run) for draws at the ends of u1 and u2, with five or more redraws,
and within 1e-6 of the 85 degree threshold on either side; (kind, step, particle, case).  Regenerate with
``python tools/find_draws.py --seed 0x1234ABCD5678 --draws 8000000``.  test_table_is_what_it_says re-derives every entry,
so a stale table fails here, on the CPU.

The two figures that the GPU test's tolerances are derived from are measured here, printed, and held under the literals
MIRROR_DIR_ERR and MIRROR_GAP_ERR (tests/test_gpu_draws.py multiplies them by 16)."""
import math
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from argon_monte_carlo_amd import params as PR  # noqa: E402
from argon_monte_carlo_amd.energised import CASES, GAP_CASE  # noqa: E402
from tests import draw_ref as R  # noqa: E402
from tests import edge_states as E  # noqa: E402
from tests import philox_ref  # noqa: E402

SEED = 0x1234abcd5678
TABLE = (
    ('u1_lo', 0x07cfd317, 717, 4),
    ('u1_lo', 0x1bd1e907, 490, 7),
    ('u1_hi', 0x0afe04d7, 1051, 3),
    ('u1_hi', 0x1133d3b4, 752, 4),
    ('u2_lo', 0x2b2f7246, 1191, 3),
    ('u2_lo', 0x3740f730, 185, 4),
    ('u2_hi', 0x0d0ff476, 808, 4),
    ('u2_hi', 0x27509b51, 663, 6),
    ('redraws', 0x28cfb850, 941, 4),
    ('redraws', 0x3531f2eb, 82, 6),
    ('near_reject', 0x1c5581d4, 533, 3),
    ('near_reject', 0x1891921a, 794, 4),
    ('near_accept', 0x0158885c, 339, 4),
    ('near_accept', 0x16d6cff1, 302, 3),
    ('near_flip', 0x0e8f1175, 969, 4),
    ('near_flip', 0x3cde1cb9, 1097, 6),
    ('high_step', 0x20000000, 0, 3),
    ('high_step', 0x3fffffff, 6, 7),
)
STEPS = (0,) + tuple(e[1] for e in TABLE)          # the bulk step and one step per entry: what the GPU test runs
PLANE_NORMAL = {3: (0.0, 0.0, 1.0), 4: (0.0, 0.0, -1.0), 6: (0.0, 0.0, 1.0), 7: (0.0, 0.0, -1.0)}
NEAR_KINDS = ("near_reject", "near_accept", "near_flip")
MARGIN, BAND = 1.0e-12, 1.0e-6
# measured here (test_mirror_against_40_digits, test_gap_energy_mirrors): the float64 mirrors against the 40-digit references
MIRROR_DIR_ERR = 3.4e-16          # largest absolute component error of a direction (measured 3.33e-16)
MIRROR_GAP_ERR = 8.0e-16          # largest relative error of gap_energy_gl(n_gl = 32) over the ladder (measured 7.96e-16)
KS_BOUND = math.sqrt(math.log(2.0e9) / 2.0)          # D sqrt(n) < 3.27: a false alarm of 1e-9 (and the draws are fixed)

_CACHE = {}


def state():
    """(temp_draw_hits() with the params a context needs, constants, E_cold, E_hot)"""
    if "state" not in _CACHE:
        from argon_monte_carlo_amd.energised import SurfaceEnergies
        s = E.temp_draw_hits()
        c = PR.pore_params(n=s.n, energised=True)[1]
        en = SurfaceEnergies(c)
        s.p.reserved0 |= 1
        s.p.E_cold, s.p.E_hot = en.cold, en.hot          # Temp:83-84 (what the device uses for the coated walls)
        _CACHE["state"] = (s, c, en)
    return _CACHE["state"]


def oracle_of(s):
    from oracle import oracle as O
    orc = O.Oracle(s.p, mode="mul")
    a = s.arrays()
    orc.upload(*a[:10], flag=a[10])
    return orc


def reference(step, case, idx, normals):
    """draw_ref.reference of the hits (idx, normals) of one case at one step; computed once per distinct input"""
    idx, normals = np.ascontiguousarray(idx, dtype=np.int64), np.ascontiguousarray(normals, dtype=np.float64)
    key = (step, case, idx.tobytes(), normals.tobytes())
    if key not in _CACHE:
        _CACHE[key] = R.reference(SEED, idx, step, case, normals)
    return _CACHE[key]


def oracle_step(step):
    """The oracle through the state's first step with the 40-digit reference's directions (rounded to double) and the
    float64 gap energies: {case: (idx, normals, contact z, ok, reference of the ok hits)}; computed once per step."""
    key = ("oracle", step)
    if key in _CACHE:
        return _CACHE[key]
    s, c, en = state()
    orc = oracle_of(s)
    orc._temp_wall_count = orc._temp_errs = 0
    orc.drift(s.dt, True)
    orc.temp_specular()
    out = {}
    for case in CASES:
        idx, nm, cz, ok = orc.wall_hits(case)
        ok = np.asarray(ok, dtype=bool)
        ref = reference(step, case, idx[ok], nm[ok])
        dirs, Es = np.zeros((len(idx), 3)), np.zeros(len(idx))
        dirs[ok] = ref["dir"]
        Es[ok] = [R.gap_energy_gl(z, c, 32) for z in cz[ok]] if case == GAP_CASE else (en.cold if case in (3, 7, 9) else en.hot)
        orc.wall_apply(case, dirs, Es)
        out[case] = (idx, nm, cz, ok, ref)
    _CACHE[key] = out
    return out


def entry_draw(step, particle, case):
    return R.mirror(SEED, [particle], step, case, PLANE_NORMAL[case])


# ---- the generator and the recipe ----------------------------------------------------------------------------------------
def test_numpy_philox_equals_the_plain_python_one():
    rs = np.random.RandomState(5)
    ctr = rs.randint(0, 1 << 32, size=(3000, 4), dtype=np.uint64)
    ctr[:8] = [[0, 0, 0, 0], [0xFFFFFFFF] * 4, [1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1],
               [0xFFFFFFFF, 0, 0xFFFFFFFF, 0], [0, 0x3FFFFFFF, (9 << 16) | 4095, R.TAG]]
    seeds = [0, SEED, 0xFFFFFFFFFFFFFFFF, 0x243F6A8885A308D3]
    for seed in seeds:
        w = R.philox(ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3], seed)
        got = np.stack(w, axis=1)
        want = [philox_ref.philox4x32_10(row.tolist(), [seed & 0xFFFFFFFF, seed >> 32]) for row in ctr]
        assert np.array_equal(got, np.array(want, dtype=np.uint64)), hex(seed)


def test_mirror_forms_the_numbers_as_direction_draw_does():
    rs = np.random.RandomState(6)
    n = 2000
    particle, step = rs.randint(0, 1 << 31, n), rs.randint(0, 1 << 30, n)
    case, attempt = rs.randint(3, 10, n), rs.randint(0, 4096, n)
    u1, u2, sign, _ = R.uniforms(SEED, particle, step, case, attempt)
    ct, phi, _ = R.components(u1, u2, sign)
    for k in range(n):
        want = philox_ref.direction_draw(SEED, int(particle[k]), int(step[k]), int(case[k]), int(attempt[k]))
        assert (ct[k], phi[k], sign[k]) == want, k


def test_cos85_is_the_double_of_the_reference_expression():
    """Temp:136 compares with cos(85 * pi / 180) as Python evaluates it: 0x1.64fd6b8c28100p-4, 2 ulp below the correctly
    rounded cosine of 85 degrees.  The kernel's literal, the library's host helper and the tests use that double."""
    assert R.COS85 == float.fromhex("0x1.64fd6b8c28100p-4") == PR.pore_params(n=0, energised=True)[0].cos85
    src = open(os.path.join(ROOT, "argon_monte_carlo_amd", "csrc", "amc_energised_dev.h")).read()
    assert "const double cos85 = 0x1.64fd6b8c28100p-4;" in src


# ---- the table ------------------------------------------------------------------------------------------------------------
def test_table_is_what_it_says():
    s = state()[0]
    kinds = {}
    for kind, step, particle, case in TABLE:
        assert 0 <= step <= 0x3FFFFFFF and particle in s.cases[f"draw_case{case}"], (kind, step, particle, case)
        m = entry_draw(step, particle, case)
        w = m["walked"]
        gap = np.abs(w[:, 4]) - R.COS85
        band = (np.abs(gap) > MARGIN) & (np.abs(gap) < BAND)
        last = w[:, 1] == m["attempts"][0]
        holds = {"u1_lo": m["u1"][0] < 1e-6, "u1_hi": m["u1"][0] > 1 - 1e-6, "u2_lo": m["u2"][0] < 1e-6, "u2_hi": m["u2"][0] > 1 - 1e-6,
                 "redraws": m["attempts"][0] >= 5, "near_reject": bool((band & (gap < 0)).any()),
                 "near_accept": bool((band & last & (gap > 0)).any()) and not m["flip"][0],
                 "near_flip": bool((band & last & (gap > 0)).any()) and bool(m["flip"][0]), "high_step": step >= 1 << 29}[kind]
        assert holds, (kind, hex(step), particle, case)
        kinds[kind] = kinds.get(kind, 0) + 1
    assert set(kinds) == {"u1_lo", "u1_hi", "u2_lo", "u2_hi", "redraws", "near_reject", "near_accept", "near_flip", "high_step"}
    assert min(kinds.values()) >= 2 and 0x3FFFFFFF in STEPS and len(set(STEPS)) == len(STEPS) <= 25


# ---- the mirrors against 40 digits -----------------------------------------------------------------------------------------
def test_mirror_against_40_digits(capsys):
    """2,000 bulk draws (all seven cases, normals all round the sphere) and every table entry: the float64 mirror takes the
    reference's decisions, and its direction lies within MIRROR_DIR_ERR of the reference's in every component."""
    rs = np.random.RandomState(7)
    n = 2000
    particle, step, case = rs.randint(0, 1 << 20, n), rs.randint(0, 1 << 30, n), rs.randint(3, 10, n)
    normal = rs.standard_normal((n, 3))
    normal[::3, 2] = 0.0                                                # cylinder normals
    normal[1::3, :2] = 0.0                                              # plane normals
    normal /= np.linalg.norm(normal, axis=1)[:, None]
    for kind, st, pa, ca in TABLE:
        particle, step, case = np.append(particle, pa), np.append(step, st), np.append(case, ca)
        normal = np.vstack([normal, PLANE_NORMAL[ca]])
    m = R.mirror(SEED, particle, step, case, normal)
    ref = R.reference(SEED, particle, step, case, normal)
    close = ref["margins"][ref["margins"][:, 2] <= MARGIN]
    assert not len(close), close                                     # (else the decision may be rounding's, not the mirror's)
    for k in ("attempts", "flip", "sign", "u1", "u2"):
        assert np.array_equal(m[k], ref[k]), k
    err = float(np.abs((m["dir"] - ref["dir"]) - ref["dir_lo"]).max())
    with capsys.disabled():
        print(f"\n[draws] float64 mirror vs 40 digits, {len(particle)} draws: largest component error {err:.3g} "
              f"(literal {MIRROR_DIR_ERR:.3g}, device tolerance {16 * MIRROR_DIR_ERR:.3g})")
    assert err <= MIRROR_DIR_ERR <= 1e-13 / 16


def test_gap_energy_mirrors(capsys):
    """gap_energy_gl against gap_energy_ref over the ladder for n_gl = 4, 8, 32, and SurfaceEnergies.gap against the same."""
    s, c, en = state()
    zs = E.draw_ladder_z(s.p)
    refs = [R.gap_energy_ref(z, c) for z in zs]
    worst = {n_gl: max(R.rel_err(R.gap_energy_gl(z, c, n_gl), r) for z, r in zip(zs, refs)) for n_gl in (4, 8, 32)}
    host = max(R.rel_err(en.gap(z), r) for z, r in zip(zs[:4] + zs[4::10], refs[:4] + refs[4::10]))
    with capsys.disabled():
        print(f"\n[draws] Gauss-Legendre mirror vs 40 digits over {len(zs)} ladder points: " +
              ", ".join(f"n_gl={k} {v:.3g}" for k, v in worst.items()) +
              f"; SurfaceEnergies.gap {host:.3g} (literal {MIRROR_GAP_ERR:.3g}, device tolerance {16 * MIRROR_GAP_ERR:.3g})")
    assert worst[32] <= MIRROR_GAP_ERR <= 1e-12 / 16
    assert 1e-7 < worst[4] < 1e-5 and 1e-14 < worst[8] < 1e-12          # the rules differ by far more than the tolerance
    assert host < 1e-14


# ---- the recipe is the distribution it claims --------------------------------------------------------------------------------
def ks(x, lo, hi):
    x = np.sort((np.asarray(x) - lo) / (hi - lo))
    n = len(x)
    return max((np.arange(1, n + 1) / n - x).max(), (x - np.arange(n) / n).max()) * math.sqrt(n)


@pytest.mark.parametrize("case, normal", [(3, (0.0, 0.0, 1.0)), (4, (0.0, 0.0, -1.0)), (5, (0.0, -1.0, 0.0)),
                                          (9, (-math.cos(1.1), -math.sin(1.1), 0.0))])
def test_recipe_is_uniform_on_the_cap(capsys, case, normal):
    """100,000 mirror draws: d.n uniform on [cos85, 1] (a Lambert-free, area-uniform cap as Temp:119-141 has it) and the
    azimuth about n uniform on the circle; Kolmogorov-Smirnov, D sqrt(n) < 3.27."""
    n = 100_000
    k = np.arange(n)
    nrm = np.array(normal)
    m = R.mirror(SEED, k % 4096, k // 4096, case, nrm)
    f = m["dir"]
    a = np.array([0.0, 0.0, 1.0]) if abs(nrm[2]) < 0.9 else np.array([1.0, 0.0, 0.0])
    e1 = np.cross(nrm, a)
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(nrm, e1)
    d_cap, d_az = ks(f @ nrm, R.COS85, 1.0), ks(np.arctan2(f @ e2, f @ e1), -math.pi, math.pi)
    with capsys.disabled():
        print(f"\n[draws] case {case} normal {normal}: KS d.n {d_cap:.2f}, azimuth {d_az:.2f} (bound {KS_BOUND:.2f})")
    assert d_cap < KS_BOUND and d_az < KS_BOUND
    assert 0.07 < (m["attempts"] > 0).mean() < 0.11 and 0.45 < m["flip"].mean() < 0.55 and 0.45 < (m["sign"] > 0).mean() < 0.55


def test_a_53_bit_u2_shows_in_the_bit_statistic():
    """draw_ref.u2_bit_statistic on the mirror is zero to 1e-18; on a mirror that keeps 53 bits of words 2 and 3 it is
    2^-53.  The GPU test asks |statistic| < 2^-54 of the device."""
    k = np.arange(4000)
    ref = reference(0, 3, k, np.tile([0.0, 0.0, 1.0], (len(k), 1)))
    w3 = R.uniforms(SEED, k, 0, 3, ref["attempts"])[3]
    good, n_used = R.u2_bit_statistic(R.mirror(SEED, k, 0, 3, [0.0, 0.0, 1.0])["dir"], ref, w3)
    bad, _ = R.u2_bit_statistic(R.mirror(SEED, k, 0, 3, [0.0, 0.0, 1.0], u2_shift=11)["dir"], ref, w3)
    assert n_used > 3000 and abs(good) < 2.0 ** -57 and abs(bad - 2.0 ** -53) < 2.0 ** -57, (good, bad)


# ---- the state ---------------------------------------------------------------------------------------------------------------
def test_state_through_the_oracle_with_host_draws():
    """temp_draw_hits() through one step of the oracle's own host loop: at least 150 hits of every case, each particle hit
    once but the corner particles (cases 4 and 8), the ladder's contact z the uploaded z bit for bit, everything finite."""
    from argon_monte_carlo_amd.energised import DirectionSampler
    s, c, en = state()
    assert 1300 <= s.n <= 1600 and len(s.cases["draw_ladder"]) == E.DRAW_LADDER
    assert not np.any(np.abs(np.stack([s.vx, s.vy, s.vz])) > 1e5)          # no overflowing particle
    orc = oracle_of(s)
    seen = {}
    orig = orc.wall_hits

    def wall_hits(case):
        r = orig(case)
        seen.setdefault(case, r)
        return r
    orc.wall_hits = wall_hits
    rc, *_ = orc.temp_timestep(s.dt, DirectionSampler(np.random.RandomState(17), random.Random(17)), en)
    assert rc == 0
    hits = np.zeros(s.n, dtype=int)
    for case in CASES:
        idx, nm, cz, ok = seen[case]
        assert len(idx) >= 150, (case, len(idx))
        np.add.at(hits, idx, 1)
        if case in PLANE_NORMAL:
            assert (nm == np.array(PLANE_NORMAL[case])).all(), case
        else:
            good = nm[np.asarray(ok, dtype=bool)]
            on_axis = (good[:, 0] == 0.0) | (good[:, 1] == 0.0)
            assert on_axis.sum() >= 4 and len(np.unique(np.round(np.arctan2(good[:, 1], good[:, 0]), 3))) >= 150, case
        if case == GAP_CASE:
            ladder = np.isin(idx, s.cases["draw_ladder"])
            assert ladder.sum() == E.DRAW_LADDER
            assert np.array_equal(cz[ladder].view(np.uint64), s.z[idx[ladder]].view(np.uint64))
            assert sorted(cz[ladder].tolist()) == sorted(E.draw_ladder_z(s.p))
    corners = np.array(s.cases["draw_corner_4_8"])
    assert (hits[corners] == 2).all() and (np.delete(hits, corners) == 1).all()
    st = orc.state()
    for k in ("x", "y", "z", "vx", "vy", "vz", "d", "dx", "dy", "dz"):
        assert np.isfinite(st[k]).all(), k
    assert s.flag.min() == 0 and s.flag.max() == 1


# ---- the margin condition -------------------------------------------------------------------------------------------------------
def test_no_decision_hangs_on_rounding():
    """For SEED and every step the GPU test runs, with the oracle's normals: no attempt of any hit has | |d.n| - cos85 | <=
    1e-12, so a device whose libm rounds otherwise takes the same decisions; the table's near-threshold entries are the only
    attempts inside 1e-6.  (A step that breaks this is replaced by another: tools/find_draws.py --skip-step.)"""
    near = {(step, particle, case) for kind, step, particle, case in TABLE if kind in NEAR_KINDS}
    worst, inside, total = 1.0, set(), 0
    for step in STEPS:
        for case, (idx, nm, cz, ok, ref) in oracle_step(step).items():
            mg, good = ref["margins"], idx[ok]
            total += len(mg)
            worst = min(worst, float(mg[:, 2].min()))
            inside |= {(step, int(good[int(h)]), case) for h in mg[mg[:, 2] < BAND, 0]}
    assert worst > MARGIN, worst
    assert inside == near, (inside ^ near)
    assert total > 1400 * len(STEPS)


def test_reference_covers_every_kind_of_draw():
    """Over the steps the GPU test runs the reference has, in every case: flipped and unflipped hits, both signs, hits with
    one redraw and with two or more."""
    for case in CASES:
        att = np.concatenate([oracle_step(step)[case][4]["attempts"] for step in STEPS])
        flip = np.concatenate([oracle_step(step)[case][4]["flip"] for step in STEPS])
        sign = np.concatenate([oracle_step(step)[case][4]["sign"] for step in STEPS])
        for what in (flip, ~flip, sign > 0, sign < 0, att == 0, att == 1, att >= 2):
            assert what.sum() >= 5, (case, what.sum())
