"""Host (no GPU): the references that tests/test_gpu_wall_law.py holds the Maxwell wall law of the device-RNG energised pore
against (tests/wall_law_ref.py; include/argonmc-walllaw.h), the table of chosen step words, the law's statistics
on the float64 mirror, the ends of the uniforms, and the ABI.

The table: tools/find_wall_law_draws.py searched the draws of SEED over find_draws.py's sequence of steps in [0, 2^30) and the
particles of edge_states.temp_draw_hits() for the smallest and the largest ua and ub of a diffuse hit and for u0 closest to
either alpha on either side; (kind, step, particle, case).  Regenerate with
``python tools/find_wall_law_draws.py --seed 0x1234ABCD5678 --alpha-coated 0.95 --alpha-gap 0.8 --draws 4000000``.
test_table_is_what_it_says re-derives every entry.  The largest step word is 0x3fffffff: amc_set_step admits no larger one.

The figure that the GPU test's velocity tolerance is derived from is measured here, printed, and held under the literal
MIRROR_VEL_ERR (tests/test_gpu_wall_law.py multiplies it by 16, the factor of tests/test_gpu_draws.py)."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from argon_monte_carlo_amd import _abi, _lib  # noqa: E402
from argon_monte_carlo_amd import params as PR  # noqa: E402
from tests import draw_ref as R  # noqa: E402
from tests import edge_states as E  # noqa: E402
from tests import wall_law_ref as W  # noqa: E402

SEED, ALPHA_COATED, ALPHA_GAP = 0x1234abcd5678, 0.95, 0.8
TABLE = (
    ('ua_lo', 0x0bf98909, 366, 5),
    ('ua_hi', 0x350e49a2, 574, 7),
    ('ub_lo', 0x20df274a, 290, 4),
    ('ub_hi', 0x2b476e27, 148, 3),
    ('coated_below', 0x0f8d8101, 623, 7),
    ('coated_above', 0x12caec94, 1095, 4),
    ('gap_below', 0x135dbf34, 933, 5),
    ('gap_above', 0x364572fe, 1115, 5),
    ('high_step', 0x20000000, 0, 3),
    ('high_step', 0x3fffffff, 674, 5),
)
STEPS = (0,) + tuple(e[1] for e in TABLE)          # the bulk step and one step per entry: what the GPU test runs
# measured here (test_mirror_against_40_digits): the float64 mirror against the 40-digit reference, velocity components over s
MIRROR_VEL_ERR = 1.4e-15          # (measured 1.32e-15 over 4,420 hits)

_CACHE = {}


def consts():
    """(params, constants, draw_ref.gap_consts, argon mass) of the energised pore"""
    if "c" not in _CACHE:
        p, c = PR.pore_params(n=1330, energised=True)
        _CACHE["c"] = (p, c, R.gap_consts(c), float(p.argon_mass))
    return _CACHE["c"]


def s_of(t_w):
    p, c, g, m = consts()
    return math.sqrt(g["boltzman"] * t_w / m)


# ---- the table ------------------------------------------------------------------------------------------------------------------
def test_table_is_what_it_says():
    s = E.temp_draw_hits()
    kinds = set()
    for kind, step, particle, case in TABLE:
        names = [f"draw_case{case}"] + (["draw_ladder"] if case == 5 else [])
        assert 0 <= step <= 0x3FFFFFFF and any(particle in s.cases[k] for k in names), (kind, step, particle, case)
        u0, ua, ub, uc = (float(a[0]) for a in W.uniforms(SEED, [particle], step, case))
        alpha = ALPHA_GAP if case == 5 else ALPHA_COATED
        holds = {"ua_lo": u0 < alpha and ua < 1e-6, "ua_hi": u0 < alpha and ua > 1 - 1e-6, "ub_lo": u0 < alpha and ub < 1e-6,
                 "ub_hi": u0 < alpha and ub > 1 - 1e-6, "coated_below": case != 5 and 0 < alpha - u0 < 1e-7,
                 "coated_above": case != 5 and 0 <= u0 - alpha < 1e-7, "gap_below": case == 5 and 0 < alpha - u0 < 1e-5,
                 "gap_above": case == 5 and 0 <= u0 - alpha < 1e-5, "high_step": step >= 1 << 29}[kind]
        assert holds, (kind, hex(step), particle, case, u0, ua, ub)
        kinds.add(kind)
    assert kinds == {"ua_lo", "ua_hi", "ub_lo", "ub_hi", "coated_below", "coated_above", "gap_below", "gap_above", "high_step"}
    assert 0x3FFFFFFF in STEPS and len(set(STEPS)) == len(STEPS) <= 16


def test_uniforms_are_the_recipes_words():
    """u0, ua from words (0, 1) and (2, 3) of the call with j = 0, ub, uc of the call with j = 1, 53 bits each, under the tag
    "AMC2" — restated here with Python integers on draw_ref.philox."""
    rs = np.random.RandomState(11)
    n = 500
    particle, step, case = rs.randint(0, 1 << 31, n), rs.randint(0, 1 << 30, n), rs.randint(3, 10, n)
    got = W.uniforms(SEED, particle, step, case)
    assert W.TAG == int.from_bytes(b"AMC2", "big") == 0x414d4332 and W.TAG != R.TAG
    for k in range(n):
        want = []
        for j in (0, 1):
            w = [int(a[0]) for a in R.philox([int(particle[k])], [int(step[k])], [(int(case[k]) << 16) | j], [W.TAG], SEED)]
            want += [float(((w[0] << 32 | w[1]) >> 11)) * 2.0 ** -53, float(((w[2] << 32 | w[3]) >> 11)) * 2.0 ** -53]
        assert [float(a[k]) for a in got] == want, k
    assert all(0.0 <= float(a.min()) and float(a.max()) < 1.0 for a in got)


# ---- the mirror against 40 digits -----------------------------------------------------------------------------------------------
def test_mirror_against_40_digits(capsys):
    """630 hits of every case — plane normals (0, 0, +-1), cylinder normals all round the circle (the four axes included), gap
    contacts across the gap and on both of its planes, incoming velocities of the gas's size — at alpha 0.95 / 0.8, and every
    table entry: the mirror takes the reference's decisions (they are exact comparisons) and every velocity component lies
    within MIRROR_VEL_ERR * s of the reference's."""
    p, c, g, m = consts()
    rs = np.random.RandomState(12)
    per = 630
    cases = np.repeat(np.arange(3, 10), per)
    n = len(cases)
    particle, step = rs.randint(0, 1 << 20, n), rs.randint(0, 1 << 30, n)
    ang = np.concatenate([[0.0, 0.5 * np.pi, np.pi, 1.5 * np.pi], rs.uniform(0, 2 * np.pi, per - 4)])
    normal = np.zeros((n, 3))
    for case in range(3, 10):
        sel = cases == case
        if case in W.PLANE_CASES:
            normal[sel, 2] = 1.0 if case in (3, 6) else -1.0
        else:
            normal[sel, 0], normal[sel, 1] = -np.cos(ang), -np.sin(ang)
    normal[np.abs(normal) < 1e-15] = 0.0
    cz = np.where(cases == 5, p.t_zgap_lo + (p.t_zgap_hi - p.t_zgap_lo) * np.concatenate([[0.0, 1.0], rs.uniform(0, 1, n - 2)]), 1.0e-7)
    v = rs.standard_normal((n, 3)) * 300.0
    for kind, st, pa, ca in TABLE:
        particle, step, cases = np.append(particle, pa), np.append(step, st), np.append(cases, ca)
        normal = np.vstack([normal, (0.0, 0.0, 1.0) if ca in W.PLANE_CASES else (0.0, -1.0, 0.0)])
        cz, v = np.append(cz, 0.5 * (p.t_zgap_lo + p.t_zgap_hi)), np.vstack([v, (120.0, -340.0, 410.0)])
    mir = W.mirror(SEED, particle, step, cases, normal, cz, v, ALPHA_COATED, ALPHA_GAP, g, m)
    ref = W.reference(SEED, particle, step, cases, normal, cz, v, ALPHA_COATED, ALPHA_GAP, g, m)
    assert np.array_equal(mir["diffuse"], ref["diffuse"]) and ref["margin"].min() > 0.0
    assert 0.9 < ref["diffuse"][cases != 5].mean() < 0.99 and 0.7 < ref["diffuse"][cases == 5].mean() < 0.9
    err = np.abs((mir["w"] - ref["w"]) - ref["w_lo"]) / ref["s"][:, None]
    worst = float(err.max())
    with capsys.disabled():
        print(f"\n[wall law] float64 mirror vs 40 digits, {len(cases)} hits: largest velocity component error {worst:.3g} s "
              f"(diffuse {float(err[ref['diffuse']].max()):.3g}, specular {float(err[~ref['diffuse']].max()):.3g}; literal "
              f"{MIRROR_VEL_ERR:.3g}, device tolerance {16 * MIRROR_VEL_ERR:.3g})")
    assert worst <= MIRROR_VEL_ERR <= 1e-13 / 16


# ---- the law's statistics -------------------------------------------------------------------------------------------------------
N_STAT = 200_000
KINDS = {"plane": (3, (0.0, 0.0, 1.0)), "cylinder": (9, (-math.cos(1.1), -math.sin(1.1), 0.0)), "gap": (5, (0.0, -1.0, 0.0))}


def moments(kind, wrong=None):
    """name -> (value, expectation, standard error) over N_STAT mirror draws of one surface kind at fixed seeds."""
    p, c, g, m = consts()
    case, normal = KINDS[kind]
    k = np.arange(N_STAT)
    cz = p.t_zgap_lo + (p.t_zgap_hi - p.t_zgap_lo) * ((k * 0.6180339887498949) % 1.0)
    mir = W.mirror(SEED, k % 4096, k // 4096, case, normal, cz, (100.0, 200.0, -300.0), ALPHA_COATED, ALPHA_GAP, g, m, wrong=wrong)
    alpha = ALPHA_GAP if case == 5 else ALPHA_COATED
    d = mir["diffuse"]
    nd = int(d.sum())
    w, s, nrm = mir["w"][d], mir["s"][d], np.array(normal)
    if case in W.PLANE_CASES:
        a, t1, t2 = w[:, 2] * nrm[2], w[:, 0], w[:, 1]
    else:
        a, t1, t2 = w[:, 0] * nrm[0] + w[:, 1] * nrm[1], -w[:, 0] * nrm[1] + w[:, 1] * nrm[0], w[:, 2]
    a, t1, t2 = a / s, t1 / s, t2 / s
    e = 0.5 * (a * a + t1 * t1 + t2 * t2)                    # E' / (k T_w)
    cos = a / np.sqrt(a * a + t1 * t1 + t2 * t2)
    r = 1.0 / math.sqrt(nd)
    return {"share": (nd / N_STAT, alpha, math.sqrt(alpha * (1 - alpha) / N_STAT)),
            "vn2": (float((a * a).mean()), 2.0, 2.0 * r), "t1_2": (float((t1 * t1).mean()), 1.0, math.sqrt(2.0) * r),
            "t2_2": (float((t2 * t2).mean()), 1.0, math.sqrt(2.0) * r), "t1": (float(t1.mean()), 0.0, r), "t2": (float(t2.mean()), 0.0, r),
            "energy": (float(e.mean()), 2.0, math.sqrt(2.0) * r), "cos": (float(cos.mean()), 2.0 / 3.0, math.sqrt(1.0 / 18.0) * r),
            "outward": (float((a < 0).sum()), 0.0, 0.5)}


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_law_statistics_on_the_mirror(capsys, kind):
    """200,000 mirror draws per surface kind at fixed seeds (deterministic), in units of the hit's own s = sqrt(k T_w / m) — on
    the gap wall T_w changes from hit to hit.  With E1, E2 independent unit exponentials the law says (w.n)^2 = 2 s^2 E1,
    t1^2 + t2^2 = 2 s^2 E2 with a uniform angle, so over the n_d diffuse hits of N draws:
      diffuse share          alpha                 standard error sqrt(alpha (1 - alpha) / N)       (a Bernoulli variable)
      <(w.n)^2> / s^2        2                     2 / sqrt(n_d)                                    (Var 2 E1 = 4)
      <t1^2>, <t2^2> / s^2   1                     sqrt(2 / n_d)                                    (Var z^2 = 2 for a unit normal z)
      <t1>, <t2> / s         0                     1 / sqrt(n_d)
      <E'> / (k T_w)         2                     sqrt(2 / n_d)                                    (E' = k T_w (E1 + E2), Var = 2)
      <cos theta>            2 / 3                 sqrt(1 / (18 n_d))                               (cos^2 = E1 / (E1 + E2) is uniform)
    Each within five standard errors, and no diffuse velocity points into the wall.  The half-Gaussian recipe (vn without the
    flux weighting: <(w.n)^2> = s^2, <E'> = 1.5 k T_w, <cos> = 0.4817) fails the same bounds."""
    got = moments(kind)
    with capsys.disabled():
        print(f"\n[wall law] {kind}: " + ", ".join(f"{k} {(v - x) / se:+.2f} se" for k, (v, x, se) in got.items() if k != "outward"))
    for name, (value, expect, se) in got.items():
        assert abs(value - expect) <= 5.0 * se, (kind, name, value, expect, se)
    bad = moments(kind, wrong="half_gaussian")
    failed = {name for name, (value, expect, se) in bad.items() if abs(value - expect) > 5.0 * se}
    assert {"vn2", "energy", "cos"} <= failed and "share" not in failed, (kind, failed)


# ---- the ends of the uniforms, and the specular formula -------------------------------------------------------------------------
def test_ends_of_the_uniforms():
    """ua = 0 gives vn = 0 (ub = 0: no tangential speed; both: a particle at rest, whose recorded direction is zero); the
    largest uniform, 1 - 2^-53, gives the largest speed: finite and below 2^14 m/s at the pore's hottest wall, so every sampler's
    velocity range holds."""
    p, c, g, m = consts()
    top = 1.0 - 2.0 ** -53
    t_max = max(g["t_cold"], g["t_hot"])
    s = s_of(t_max)
    for normal, cyl in (((0.0, 0.0, -1.0), False), ((-0.6, -0.8, 0.0), True)):
        nrm = np.array([normal])
        w = W.emit([0.0], [0.3], [0.2], [s], nrm, [cyl])[0]
        # (exactly zero on a plane; on a cylinder the two products t1 n1 n0 and t1 n0 n1 round on their own)
        assert abs(float(w @ nrm[0])) <= (4 * 2.0 ** -53 * np.linalg.norm(w) if cyl else 0.0) and np.linalg.norm(w) > 0
        w = W.emit([0.0], [0.0], [0.2], [s], nrm, [cyl])
        assert not w.any()
        d, dpz, dE = W.finish(np.array([[10.0, 20.0, 30.0]]), w, m)
        assert not d.any() and np.isfinite([dpz[0], dE[0]]).all() and dE[0] == -0.5 * m * (math.sqrt(1400.0) * math.sqrt(1400.0))
        for uc in (0.0, 0.125, 0.25, 0.5, top):
            w = W.emit([top], [top], [uc], [s], nrm, [cyl])[0]
            speed = float(np.linalg.norm(w))
            assert np.isfinite(w).all() and speed < 2.0 ** 14 and np.abs(w).max() < 2.0 ** 14, (normal, uc, speed)
            assert abs(float(w @ nrm[0]) / s - math.sqrt(2 * 53 * math.log(2.0))) < 1e-12
    assert 12.0 * s < 2.0 ** 14 and math.sqrt(2.0) * math.sqrt(2 * 53 * math.log(2.0)) < 12.2


def test_specular_conserves_speed_and_reverses_the_normal_component():
    rs = np.random.RandomState(13)
    n = 5000
    ang = rs.uniform(0, 2 * np.pi, n)
    normal = np.stack([-np.cos(ang), -np.sin(ang), np.zeros(n)], axis=1)
    normal[::2] = [0.0, 0.0, 1.0]
    normal[1::4] = [0.0, 0.0, -1.0]
    v = rs.standard_normal((n, 3)) * 400.0
    w = W.specular(v, normal)
    vmag = np.linalg.norm(v, axis=1)
    assert np.abs(np.linalg.norm(w, axis=1) / vmag - 1.0).max() < 8 * 2.0 ** -53
    assert np.abs(((w * normal).sum(axis=1) + (v * normal).sum(axis=1)) / vmag).max() < 8 * 2.0 ** -53
    # (the tangential part, through two cross products that round on their own: a looser bound)
    tang = np.cross(normal, np.cross(v, normal))
    assert (np.abs(np.cross(normal, np.cross(w, normal)) - tang).max(axis=1) / vmag).max() < 32 * 2.0 ** -53
    plane = normal[:, 2] != 0.0                  # planes: the tangential components are untouched, bit for bit
    assert np.array_equal(w[plane, :2], v[plane, :2]) and np.array_equal(w[plane, 2], -v[plane, 2])


# ---- the ABI --------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("cc") is None, reason="no C compiler")
def test_wall_law_layout_matches_header(tmp_path):
    src = tmp_path / "layout.c"
    names = ["struct_size", "kind", "alpha_coated", "alpha_gap", "reserved"]
    body = "".join(f'    printf("{k} %zu\\n", offsetof(amc_wall_law, {k}));\n' for k in names)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "argonmc.h"\nint main(void) {\n'
                   '    printf("sizeof %zu\\n", sizeof(amc_wall_law));\n' + body +
                   '    printf("reference %d\\n", AMC_WALL_LAW_REFERENCE);\n    printf("maxwell %d\\n", AMC_WALL_LAW_MAXWELL);\n'
                   '    printf("abi %d\\n", AMC_ABI_VERSION);\n    printf("rng %zu\\n", sizeof(amc_temp_rng));\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(line.rsplit(" ", 1) for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n") if line)
    assert int(out["sizeof"]) == C.sizeof(_abi.AmcWallLaw) == 56
    for k in names:
        assert int(out[k]) == getattr(_abi.AmcWallLaw, k).offset, k
    assert int(out["reference"]) == _abi.AMC_WALL_LAW_REFERENCE == 0 and int(out["maxwell"]) == _abi.AMC_WALL_LAW_MAXWELL == 1
    assert int(out["abi"]) == 2 and int(out["rng"]) == C.sizeof(_abi.AmcTempRng)          # (amc_temp_rng is what it was)


def test_entry_points_are_declared_exported_and_typed():
    assert '#include "argonmc-walllaw.h"' in open(os.path.join(ROOT, "include", "argonmc.h")).read()
    assert os.path.join(ROOT, "include", "argonmc-walllaw.h") in _lib._source_files()
    hdr = open(os.path.join(ROOT, "include", "argonmc-walllaw.h")).read()
    names = ["amc_temp_wall_law", "amc_temp_wall_law_get"]
    assert set(re.findall(r"^int (amc_[a-z_]+)\(", hdr, flags=re.M)) == set(_lib.WALL_LAW_SIGNATURES) == set(names)
    # (beside all_signatures(), whose size tests/test_ic_separate_host.py fixes; load() types typed_signatures())
    sig = _lib.typed_signatures()
    assert set(sig) == set(_lib.all_signatures()) | set(names) and not set(names) & set(_lib.all_signatures())
    for name in names:
        assert name in sig and sig[name][0] is C.c_int and sig[name][1][1]._type_ is _abi.AmcWallLaw, name
    assert not set(_lib.WALL_LAW_SIGNATURES) & (set(sig) - set(names))
    lib = _lib.load()
    assert all(getattr(lib, name).argtypes == sig[name][1] and getattr(lib, name).restype is C.c_int for name in names)
    mk = open(os.path.join(ROOT, "argon_monte_carlo_amd", "csrc", "Makefile")).read()
    assert "argonmc-walllaw.h" in mk


def test_checkpoint_key_round_trips_through_the_array_form():
    from argon_monte_carlo_amd import energised as EN
    assert EN.WALL_LAWS == ("reference", "maxwell")
    for law in ((1, 0.95, 0.8), (1, 0.0, 1.0), (0, 0.25, 0.125), (1, 1.0 / 3.0, 2.0 ** -53)):
        arr = EN.wall_law_to_array(law)
        assert arr.dtype == np.float64 and arr.shape == (3,) and np.array_equal(arr, W.law_array(*law))
        assert EN.wall_law_from_array(arr) == law

    class FakeEngine:
        def __init__(self, law):
            self.law, self.calls = law, []

        def wall_law_get(self):
            return self.law

        def wall_law(self, kind=None, alpha_coated=None, alpha_gap=None):
            self.calls.append((kind, alpha_coated, alpha_gap))
    assert EN.wall_law_checkpoint(FakeEngine((0, 0.95, 0.8))) == {}           # the reference law: no key, as before the law existed
    ck = EN.wall_law_checkpoint(FakeEngine((1, 0.5, 0.25)))
    assert list(ck) == ["wall_law"] and ck["wall_law"].tolist() == [1.0, 0.5, 0.25]
    e = FakeEngine(None)
    EN.wall_law_restore(e, ck["wall_law"])
    EN.wall_law_restore(e, None)                                                # a file without the key
    assert e.calls == [(1, 0.5, 0.25), (None, None, None)]
    with pytest.raises(ValueError):
        EN.set_wall_law(e, None, "maxwell")                                     # no device-RNG configuration
    with pytest.raises(ValueError):
        EN.set_wall_law(e, object(), "cercignani")
    EN.set_wall_law(e, object(), "maxwell", 0.3)
    EN.set_wall_law(e, object(), None)
    assert e.calls[2:] == [(1, 0.3, None), (None, None, None)]
