"""GPU (-m gpu): the ordered resolve workgroup (k_resolve, amc_resolve.hip) at each of its size fences, on the crafted states of
tests/resolve_states.py.  Bar: bit for bit equal to the oracle (`mul`) — all eleven arrays, the collision count and the
completed paths in the reference's order for the single cells (what test_pairwise_cell_whole_cells_with_chains asserts);
state, counters and records after every stage and call for the grid states (the plan of
test_every_cluster_case_equals_the_oracle) — and, from the kernel's own debug figures (AMC_DEBUG_RESOLVE, one launch on a
fresh context: exact counts), proof that the side of the fence the state is named after was the one taken.

The oracle is pinned to the reference on the small cells by tests/test_resolve_states_host.py; the cells of RS.LARGE and
RS.FAILING are the same generators at a larger count and are compared with the oracle only.

The slot cap of the LDS label tables (pulls_2900: 5,800 slots from candidates and 2,900 claimed by the first validation,
more than the 6,144 the LDS tables hold, fewer than max_slots = 10,240) used to end in AMC_ERR_CAPACITY: the claims were
capped at the LDS tables' size.  Claims now go up to max_slots and the labels move to the work space when the slots outgrow
the LDS tables; the cell equals the oracle and the debug figures show the move."""
import re

import numpy as np
import pytest

from tests import cluster_states as CS
from tests import list_states as LS
from tests import resolve_states as RS
from tests.test_gpu_edges import Engine, O, _pair, _stagewise, _steps, assert_state_equal  # noqa: F401  (Engine, O: fixtures)

pytestmark = pytest.mark.gpu

GOOD = RS.SMALL + RS.LARGE
ON_DEMAND_STEPS = 8
FIGURES = ("rounds", "cand", "complex_last", "launches", "idle", "labels_global", "moved", "layers_lds", "split", "shared", "sorted",
           "pool_global", "sort_global", "later", "by_wave", "by_lane", "most")
LINE = re.compile(r"rounds ([\d.]+) cand ([\d.]+) complex-members ([\d.]+) launches (\d+) \(idle hand-over only (\d+)\) \| body: "
                  r"labels in the work space (\d+) moved there (\d+) layers in LDS (\d+) rounds split (\d+) heads shared (\d+) "
                  r"sorted (\d+) pool global (\d+) sort global (\d+) later (\d+) clusters by a wave (\d+) by one lane (\d+) "
                  r"most complex members (\d+)")


@pytest.fixture(scope="module")
def cells(O):
    """every cell and what the oracle makes of it, built once and left unchanged"""
    made = {}

    def get(name):
        if name not in made:
            c = RS.cell(name)
            made[name] = (c, O.pair_cell(c.p, *[c.arrays[f] for f in RS.FIELDS], mode="mul", max_records=8 * c.n))
        return made[name]
    return get


def _cell_equals(eng, c, ref, ctx):
    out, rpaths, rnc, rc = ref
    assert rc == 0
    args = c.args()
    paths, nc = eng.pairwise_cell(*args)
    assert nc == rnc > 0, (ctx, nc, rnc)
    for f, a in zip(RS.FIELDS, args):
        assert np.array_equal(a.astype(np.float64), out[f].astype(np.float64)), (ctx, f, np.flatnonzero(a != out[f])[:5])
    assert np.array_equal(paths, rpaths), ctx            # same values in the same (reference) order


def _debug_figures(eng, capfd):
    capfd.readouterr()
    eng.kernel_times()
    m = LINE.search(capfd.readouterr().err)
    assert m, "no k_resolve line"
    return {k: (float(v) if "." in v else int(v)) for k, v in zip(FIGURES, m.groups())}


def _sweep(eng, c):
    """the cell through upload / timestep(0) / download — what amc_pairwise_cell does — for the step's counters"""
    a = c.arrays
    eng.upload(a["x"], a["y"], a["z"], a["vx"], a["vy"], a["vz"], a["cont"], a["cx"], a["cy"], a["cz"], flag=a["flag"])
    st = eng.timestep(0.0)
    return st, eng.download()


def _state_equals(dev, out, ctx):
    for k, f in (("x", "x"), ("y", "y"), ("z", "z"), ("vx", "vx"), ("vy", "vy"), ("vz", "vz"), ("d", "cont"), ("dx", "cx"),
                 ("dy", "cy"), ("dz", "cz")):
        assert np.array_equal(dev[k], out[f]), (ctx, k)
    assert np.array_equal(dev["flag"].astype(bool), out["flag"].astype(bool)), ctx


# ---------------------------------------------------------------------------------------------------------------- family A
@pytest.mark.parametrize("name", [n for n in GOOD if n != "cascade_255"])
def test_every_cell_equals_the_oracle(Engine, cells, name):
    c, ref = cells(name)
    eng = Engine(c.p)
    _cell_equals(eng, c, ref, name)
    _cell_equals(eng, c, ref, (name, "again"))          # the work space of the first call is left clean for the second
    eng.close()


@pytest.mark.parametrize("name", [n for n in GOOD if n != "cascade_255"])
def test_the_intended_branch_was_taken_in_the_cell(Engine, cells, monkeypatch, capfd, name):
    """the debug instantiation on a fresh context, one launch: rounds, candidates and complex members are exact, and so are
    the counts per path, against the host-side numbers (RS.figures of the mirror's rounds)"""
    monkeypatch.setenv("AMC_DEBUG_RESOLVE", "1")        # (read at context creation)
    c, ref = cells(name)
    eng = Engine(c.p)
    _cell_equals(eng, c, ref, name)
    got = _debug_figures(eng, capfd)
    eng.close()
    want = RS.figures(RS.rounds_of(c), RS.default_capacities(c.n, c.p.max_candidates)[1])
    want.update(launches=1, idle=0, layers_lds=0)
    print(name, got)
    assert got == want, (name, {k: (got[k], want[k]) for k in want if got[k] != want[k]})
    # the side the cell is named after
    kind, _, num = name.partition("_")
    if kind == "nc":
        assert (got["split"], got["pool_global"], got["sort_global"]) == \
            (int(int(num) <= RS.RS_SPLIT), int(int(num) > RS.RS_POOL), int(int(num) > RS.RS_SORT_LDS)), (name, got)
    if kind == "heads":
        assert (got["shared"], got["by_wave"], got["by_lane"]) == (int(num == "3"), 1 + (num == "3"), 1), (name, got)
    if kind == "labels":
        assert got["labels_global"] == int(num == "2945") and got["moved"] == 0, (name, got)
    if name == "merge":
        assert got["rounds"] == 2 and got["later"] == 1 and got["complex_last"] == 14, got
    if name == "pulls_2900":
        assert (got["labels_global"], got["moved"], got["rounds"]) == (0, 1, 2), got


def test_the_cascade_needs_one_round_per_member(Engine, cells):
    """depth 2, 3 and 4 first: n_rounds is depth + 1, which is what puts cascade_255 at round 256 and cascade_256 past it"""
    for depth in (2, 3, 4, 8):
        c, (out, _, rnc, rc) = cells(f"cascade_{depth}")
        eng = Engine(c.p)
        st, dev = _sweep(eng, c)
        eng.close()
        print("cascade", depth, "n_rounds", st["n_rounds"])
        assert st["n_rounds"] == depth + 1 and st["n_pp"] == rnc, (depth, st)
        _state_equals(dev, out, ("cascade", depth))


def test_a_sweep_clean_in_round_256_is_good(Engine, cells, monkeypatch, capfd):
    """cascade_255: 256 rounds, the last one clean — equal to the oracle, n_rounds == RS_MAX_ROUNDS.  One lane emulates up to
    257 members in each round, the last one from the global working set."""
    monkeypatch.setenv("AMC_DEBUG_RESOLVE", "1")
    c, ref = cells("cascade_255")
    eng = Engine(c.p)
    st, dev = _sweep(eng, c)
    assert st["n_rounds"] == RS.RS_MAX_ROUNDS and st["n_pp"] == ref[2], st
    _state_equals(dev, ref[0], "cascade_255")
    got = _debug_figures(eng, capfd)
    print("cascade_255", got)
    want = RS.figures(RS.rounds_of(c), RS.default_capacities(c.n)[1])
    want.update(launches=1, idle=0, layers_lds=0)
    assert got == want, {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    # the completed paths in the order amc_pairwise_cell hands them out (i, j ascending, particle j before particle i)
    rec = eng.drain_paths(sort=False)
    rec = rec[np.lexsort((rec["which"], rec["j"], rec["i"]))]
    assert np.array_equal(np.stack([rec["total"], rec["px"], rec["py"], rec["pz"]], axis=1), ref[1])
    eng.close()


@pytest.mark.parametrize("name", RS.FAILING)
def test_a_sweep_beyond_the_work_space_is_reported(Engine, cells, name):
    """Round 257 still dirty | the slot table really full: the call raises AMC_ERR_CAPACITY — no hang, no crash, no silent loss
    of a collision — every time it is made, the state stays intact, and the context stays usable: a following good call on
    it equals the oracle."""
    from argon_monte_carlo_amd._lib import ArgonMCError
    c, ref = cells(name)
    assert ref[3] == 0                                  # (the reference's loop itself has no trouble with the cell)
    eng = Engine(c.p)
    for attempt in range(2 if name == "slots_full" else 1):
        args = c.args()
        with pytest.raises(ArgonMCError) as ei:
            eng.pairwise_cell(*args)
        assert ei.value.code == -4, (name, attempt, ei.value)
    st = eng.download()
    assert all(np.all(np.isfinite(st[k])) for k in ("x", "y", "z", "vx", "vy", "vz", "d"))
    for k, f in (("x", "x"), ("y", "y"), ("z", "z"), ("vx", "vx"), ("vy", "vy"), ("vz", "vz")):
        assert np.array_equal(st[k], c.arrays[f]), (name, k)            # nothing of the failed sweep was committed
    eng.drain_paths()
    good, gref = cells("nc_64")
    _cell_equals(eng, good, gref, (name, "then nc_64"))
    eng.close()


# ---------------------------------------------------------------------------------------------------------------- family B
def _grid_cases():
    for which in RS.GRID_STATES:
        for kind in CS.KINDS:
            for perm in CS.PERMS:
                for fine in RS.FINE if perm == "identity" else ("coarse",):
                    yield pytest.param(which, kind, perm, fine, id=f"{which}-{kind}-{perm}-{fine}")


def _grid_counts(s):
    st = RS.grid_structure(s)
    chains = sum(len(e["particles"]) > CS.CW_MAXM for e in st["components"])
    return len(st["pairs"]), len(st["components"]), chains


@pytest.mark.parametrize("which,kind,perm,fine", _grid_cases())
def test_every_grid_state_equals_the_oracle(Engine, O, which, kind, perm, fine):
    """one step stage by stage, then timestep x 2 and run(3); then amc_run for ON_DEMAND_STEPS steps from the fresh state,
    where the ordered workgroup is launched only after a wave of the wide kernel asked for it"""
    s = RS.grid_state(kind, perm, which)
    assert not s.extra["absent"]
    ctx = (which, kind, perm, fine)
    eng, orc = _pair(Engine, O, s, detect_mode=1, fine_cell=RS.fine_cell(s.p, fine))
    rec = _stagewise(eng, orc, s, ctx, pore=(kind == "pore"))
    assert not (rec["j"] < 0).any()
    _steps(eng, orc, s, (1, 1, 3), ctx)
    eng.close()
    s = RS.grid_state(kind, perm, which)
    eng, orc = _pair(Engine, O, s, detect_mode=1, fine_cell=RS.fine_cell(s.p, fine))
    _steps(eng, orc, s, (ON_DEMAND_STEPS,), (ctx, "run"))
    od = eng.overlap_stats()
    assert od["on_demand_steps"] >= ON_DEMAND_STEPS and od["stalls"] > 0, (ctx, od)
    eng.close()


@pytest.mark.parametrize("which,kind,perm,fine", _grid_cases())
def test_the_intended_branch_was_taken_on_the_grid(Engine, O, monkeypatch, capfd, which, kind, perm, fine):
    monkeypatch.setenv("AMC_DEBUG_RESOLVE", "1")
    s = RS.grid_state(kind, perm, which)
    ctx = (which, kind, perm, fine)
    ncand, ncomp, chains = _grid_counts(s)
    h = RS.fine_cell(s.p, fine)
    eng, orc = _pair(Engine, O, s, detect_mode=1, fine_cell=h)
    st = eng.timestep(s.dt)
    rc, so = orc.timestep(s.dt)
    assert rc == 0 and st["n_pp"] == so["n_pp"], (ctx, st, so)
    assert_state_equal(eng.download(), orc.state(), ctx)
    assert st["n_candidates"] == ncand and st["n_clusters"] == ncomp, (ctx, st, ncand, ncomp)
    got = _debug_figures(eng, capfd)
    eng.close()
    print(ctx, got)
    lds_layers = int(3 * LS.grid_of(s.p, h).gz <= RS.RS_LAY)
    nleft = 16 * chains
    assert (got["launches"], got["idle"], got["cand"], got["layers_lds"]) == (1, 0, ncand, lds_layers), (ctx, got)
    assert got["labels_global"] == int(not (2 * ncand + 2 * nleft + 256 <= RS.RS_NS)) and got["moved"] == 0, (ctx, got)
    if which.split("_")[0] in ("chains", "pairs"):
        # nothing pulls and nothing meets: one round, every chain by one lane, in the split or in the sorted path
        m = dict(rounds=1, candidates=ncand, per_round=[dict(nc=17 * chains, sizes=[17] * chains, slots=0)])
        want = RS.figures(m, RS.default_capacities(s.n)[1], wide_ns=2 * ncand, nleft=nleft)
        want.update(launches=1, idle=0, layers_lds=lds_layers)
        assert got == want, (ctx, {k: (got[k], want[k]) for k in want if got[k] != want[k]})
    else:
        # beside four chains (sorted in LDS): the workgroup's own validation, overlay and probe found what the state holds
        assert got["rounds"] >= 2 and got["later"] >= 1 and got["sorted"] >= 1 and got["most"] >= 68, (ctx, got)
