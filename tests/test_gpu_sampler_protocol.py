"""GPU (-m gpu): what every streaming sampler must do, whatever it sums — each test written once and run for the records
(tests/sampler_protocol.py) of the samplers that have it.  What only one sampler does is in tests/test_gpu_<that sampler>.py;
so are the cases of run(k) against k timesteps, each sampler's own list, over one shared body (sampler_protocol.check_run)."""
import numpy as np
import pytest

from tests import sampler_protocol as SP
from tests.sampler_protocol import KEYS
from tests.sampler_states import ODD_N, ODD_SHARDS, drifting_states

pytestmark = pytest.mark.gpu


def _records(test):
    return pytest.mark.parametrize("rec", SP.having(test), ids=lambda r: r.name)


# ---- 1. sampling changes nothing else -------------------------------------------------------------------------------------
@_records("invisible")
def test_sampling_leaves_state_counters_histograms_and_paths_unchanged(rec):
    out = []
    for on in (False, True):
        sim = SP.make_sim("pore", rec.invisible["n"], seed=5)
        if on:
            rec.enable(sim, **rec.invisible["enable"])
        stats = [sim.run(10)]
        sim._collect()
        for _ in range(10):
            stats.append(sim.timestep())
        st = sim.engine.download()
        counts, npaths = sim.engine.histograms()
        out.append((st, stats, counts, npaths, list(sim.completed_paths), list(sim.completed_x_paths)))
        if on:
            assert rec.samples(rec.read(sim.engine)) == rec.invisible["samples"]
        sim.close()
    (a, sa, ca, na, pa, pxa), (b, sb, cb, nb, pb, pxb) = out
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k
    assert sa == sb
    assert na == nb and np.array_equal(ca, cb)
    assert len(pa) > 0 and pa == pb and pxa == pxb


# ---- 2. two ranks on one GPU ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n", [("cube", 30_000), ("pore", 60_001)])
@_records("ranks")
def test_two_ranks_on_one_gpu_equal_single_engine(rec, kind, n):
    from argon_monte_carlo_amd.engine import Engine
    from tests.test_gpu_dist import _case, _run_ranks
    steps = 6
    p, c, init = _case(kind, n)
    eng = Engine(p)
    eng.upload(*init)
    rec.config(eng, rec.ranks_grid(kind, p))
    eng.run(c["dt"], steps)
    ref = rec.read(eng)
    eng.close()
    got = _run_ranks(2, (rec.name, kind, n, steps, rec.ranks["every"]), target=SP.sampler_worker)
    split = rec.sampler.split_read
    assert tuple(split(got)[2]) == split(ref)[2] and rec.samples(ref) == rec.ranks["samples"]
    assert np.array_equal(got[0], ref[0])
    if "tail" in rec.ranks:
        rec.ranks["tail"](ref, n)


# ---- 3. the walk's odd ends: an index range that begins or ends inside an aligned pair ------------------------------------------
@pytest.mark.parametrize("lo,hi", ODD_SHARDS)
@_records("odd")
def test_index_range_with_odd_ends_equals_reference(rec, lo, hi):
    """(lo odd / hi odd: the first / the last particle has no partner)"""
    from argon_monte_carlo_amd.engine import ShardEngine
    p, states = drifting_states(ODD_N, rec.odd["states"])
    eng = ShardEngine(p, lo, hi)
    rec.config(eng, rec.odd["grid"](p))
    m = rec.mirror_of(eng, hi - lo)
    for st in states:
        eng.upload(*st)
        rec.sample(eng)
        m.add(*(a[lo:hi] for a in st))
    rec.odd["tail"](eng, m, m.check(eng), states, lo, hi)
    eng.close()


# ---- 4. the shape of the shared reduce: around one workgroup of 64 columns, rows around its sixteen waves -----------------------
@pytest.mark.parametrize("rec,shape,blocks", [
    pytest.param(r, shape, blocks, id=f"{r.name}-{shape}-{blocks}") for r in SP.having("reduce") for shape in r.reduce["shapes"]
    for blocks in ("1", "17", "33")])
def test_reduce_shapes_equal_reference(rec, shape, blocks, monkeypatch):
    """1, 17 and 33 slab rows: below, one above and two above a multiple of the reduce's sixteen waves; the shapes are the
    records' (tests/sampler_protocol.py).  The second sample adds onto non-zero totals."""
    from argon_monte_carlo_amd.engine import Engine
    p, g, st, sums, *counters = SP.reduce_reference(rec, shape)
    rec.reduce["shape"](shape, g, sums, *counters)
    monkeypatch.setenv(rec.blocks, blocks)
    eng = Engine(p)
    eng.upload(*st)
    rec.config(eng, g)
    for k in (1, 2):
        rec.sample(eng)
        tot, *got = rec.read(eng)
        assert got == [k] + [k * c for c in counters]
        want = rec.reduce["words"](k * sums)
        assert np.array_equal(tot, want), np.argwhere(tot != want)[:5]
    eng.close()
