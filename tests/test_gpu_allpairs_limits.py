"""GPU (-m gpu): the two all-pairs detectors in front of the grid resolve (detect_mode = 2: k_detect_allpairs below 16384
particles, k_detect_allpairs_tiled from there on) at their tile limits, on the crafted states of tests/allpairs_states.py: a
colliding pair at in_1 .. in_8 on EVERY tile pair of the launch, at the in-tile offsets the kernels' structure makes special
(0, T - 1, the chunk boundary 7 | 8, the register rows 255 | 256 .., the last index of a partial tile), the diagonal rule
across register rows, the switch between the kernels at 16383 | 16384 | 16385, the far corner of the grid — where the
expanded form's cancellation is what the raised threshold is for — and coordinates outside the grid's extent.

Bar: state, counters and completed-path records bit-equal to the oracle (`mul`), and every crafted pair collided exactly
as its separation says (hits > 0 equals ``collide``, pair by pair).  No tolerance anywhere.  That the states reach their
edges is shown on the CPU (tests/test_allpairs_states_host.py)."""
import numpy as np
import pytest

from tests import allpairs_states as A
from tests.test_gpu_edges import COUNTERS, _pair, _stagewise, _steps, assert_records_equal, assert_state_equal

pytestmark = pytest.mark.gpu

_CACHE = {}


@pytest.fixture(scope="module")
def Engine():
    from argon_monte_carlo_amd.engine import Engine as Eng
    return Eng


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def _state(key, build):
    """the builders are deterministic: one state per key for the whole module (arrays are copied at every upload)"""
    if key not in _CACHE:
        _CACHE[key] = build()
    return _CACHE[key]


def _matrix(kind, T, ntiles, last):
    return _state(("matrix", kind, T), lambda: A.tile_matrix(kind, T, ntiles, last))


def _as_collide_says(rec, s, ctx):
    hits, _ = A.pair_hits(rec, s.extra["pairs"])
    col = s.extra["collide"]
    assert np.array_equal(hits > 0, col), (ctx, [(tuple(s.extra["pairs"][k]), s.extra["names"][k]) for k in np.flatnonzero((hits > 0) != col)[:8]])


def _one_step_by_stages(Engine, O, s, ctx, **params):
    eng, orc = _pair(Engine, O, s, detect_mode=2, **params)
    rec = _stagewise(eng, orc, s, ctx, pore=(s.extra["kind"] == "pore"))
    _as_collide_says(rec, s, ctx)
    eng.close()


def _chunks(Engine, O, s, chunks, ctx, **params):
    """a fresh engine through timestep / run chunks: the first step's records also pair by pair; returns the final arrays"""
    assert chunks[0] == 1
    eng, orc = _pair(Engine, O, s, detect_mode=2, **params)
    st = eng.timestep(s.dt)
    rc, so = orc.timestep(s.dt)
    assert rc == 0
    for key in COUNTERS:
        assert st[key] == so[key], (ctx, key, st, so)
    assert_state_equal(eng.download(), orc.state(), (ctx, "first step"))
    rec = orc.drain_paths()
    assert_records_equal(eng.drain_paths(), rec, (ctx, "first step"))
    _as_collide_says(rec, s, ctx)
    _steps(eng, orc, s, chunks[1:], ctx)
    out = eng.download()
    eng.close()
    return out


@pytest.mark.parametrize("kind,T,ntiles,last", A.MATRIX)
def test_tile_matrix(Engine, O, kind, T, ntiles, last):
    """a colliding pair on every tile pair (153, 153 and 28 of them) and a non-colliding one on every third"""
    s = _matrix(kind, T, ntiles, last)
    assert len(A.tile_pairs_covered(s)) == ntiles * (ntiles + 1) // 2 and s.extra["T"] == T
    ctx = ("tile matrix", kind, T)
    _one_step_by_stages(Engine, O, s, ctx)
    chunks = (1, 2, 1)
    final = _chunks(Engine, O, s, chunks, ctx)
    # the binned detector on the same state ends in the same arrays
    eng, _ = _pair(Engine, O, s, detect_mode=1)
    for k in chunks:
        eng.run(s.dt, k) if k > 1 else eng.timestep(s.dt)
    binned = eng.download()
    eng.close()
    for k in final:
        assert np.array_equal(final[k], binned[k]), (ctx, k)
    print(f"allpairs limits: tile_matrix {kind} T={T}: {len(s.extra['pairs'])} crafted pairs, "
          f"{len(A.tile_pairs_covered(s))} tile pairs")


def test_switch_between_the_two_kernels(Engine, O):
    """n = 16383 (the 256 kernel's largest launch), 16384 (sixteen full 1024 tiles), 16385 (a 17th tile of one particle);
    in each, one i with three hits in one chunk and one j hit from three register rows of one thread (the chunk re-walk)"""
    states = _state("switch", A.switch_sizes)
    assert [s.extra["T"] for s in states] == [A.AP_T, A.AP2_T, A.AP2_T]
    for s in states:
        ctx = ("switch", s.n)
        _one_step_by_stages(Engine, O, s, ctx)
        _chunks(Engine, O, s, (1, 2), ctx)
    print(f"allpairs limits: switch: {sum(len(s.extra['pairs']) for s in states)} crafted pairs in three states")


@pytest.mark.parametrize("kind", ["cube", "pore"])
def test_expanded_form_at_the_far_corner(Engine, O, kind):
    s = _state(("far", kind), lambda: A.far_corner(kind))
    inm = np.array([nm in A.IN for nm in s.extra["names"]])
    far = np.array(s.extra["anchor"]) == "far"
    assert (inm & far).sum() == 12 and s.extra["collide"][inm].all()
    assert (s.extra["margin"][inm] < s.extra["band"]).all()          # the pairs lie where the raised threshold decides
    ctx = ("far corner", kind)
    _one_step_by_stages(Engine, O, s, ctx)
    _chunks(Engine, O, s, (1, 2, 1), ctx)
    print(f"allpairs limits: far_corner {kind}: {len(s.extra['pairs'])} crafted pairs")


def test_tiled_detector_outside_the_grid_extent(Engine, O):
    """a sweep before walls and bounds: coordinates below z = 0, beyond R_oa and above H, outside the extent the tiled
    kernel's error bound is computed from"""
    s = _state("outside", A.outside)
    eng, orc = _pair(Engine, O, s, detect_mode=2)
    st = eng.stage_sweep()
    rc, npp, _ = orc.sweep()
    assert rc == 0 and st["n_pp"] == npp and npp > 0
    assert_state_equal(eng.download(), orc.state(), "outside")
    rec = orc.drain_paths()
    assert_records_equal(eng.drain_paths(), rec, "outside")
    hits, _ = A.pair_hits(rec, s.extra["pairs"])
    assert (hits > 0).any() and (hits == 0).any()                      # some are members of a reference cell, some not
    assert s.extra["collide"][hits > 0].all()
    eng.close()
    print(f"allpairs limits: outside: {len(s.extra['pairs'])} crafted pairs")


@pytest.mark.parametrize("knob", [{"AMC_CW_BLOCKS": "4"}, {"AMC_PLAN_SMALL": "0"}], ids=["cw_blocks", "plan_small"])
def test_tile_matrix_under_launch_knobs(Engine, O, monkeypatch, knob):
    """four waves in the wide cluster kernel; the split plan from the first sweep on"""
    for k, v in knob.items():
        monkeypatch.setenv(k, v)
    s = _matrix(*A.MATRIX[0])
    _chunks(Engine, O, s, (1, 3), ("tile matrix", tuple(knob)))
    print(f"allpairs limits: knobs {tuple(knob)}: {len(s.extra['pairs'])} crafted pairs, {len(A.tile_pairs_covered(s))} tile pairs")
