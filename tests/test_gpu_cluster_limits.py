"""GPU (-m gpu): the wide cluster kernel (k_clusters_wide, amc_clusters.hip) at each of its limits, on the crafted clusters
of tests/cluster_states.py — every one a few particles on one side of a fence written into the kernel.  Bar: bit for bit
equal to the oracle (`mul`) after every stage, in counters and in completed-path records; and for every catalogue proof, from
the oracle's records and from the kernel's own debug counters (AMC_DEBUG_RESOLVE), that the intended branch was taken.

The oracle itself is pinned to the reference on these shapes by tests/test_oracle_clusters.py.  Its results are made once
per catalogue and sequence of calls (the module-scoped ``oracles``): the first test that needs them records every call of
the oracle and what it returned, the others — the same state under another detector, grid or launch knob — replay them."""
import re

import pytest

from tests import cluster_states as CS
from tests.test_gpu_edges import Engine, O, _pair, _stagewise, _steps, assert_state_equal  # noqa: F401  (Engine, O: fixtures)

pytestmark = pytest.mark.gpu

STATES = ("within",) + CS.HANDOVER
ON_DEMAND_STEPS = 8
KINDS_WAVE = ("pair", "3-cluster", "4+-cluster", "not owner")
# what the wide kernel's first validation does with the cluster of a hand-over state (the pair beside it does nothing)
PULLS_FROM = {"full_pull": "4+-cluster", "pulls_5": "4+-cluster", "pull_depth_3": "4+-cluster", "pull_depth_4": "4+-cluster",
              "pair_pull2": "pair"}


class _Tape:
    def __init__(self):
        self.calls, self.complete = [], False


class _Recorder:
    """the oracle, every call and its result written on the tape"""

    def __init__(self, real, tape):
        self._real, self._tape = real, tape

    def __getattr__(self, name):
        f = getattr(self._real, name)

        def call(*a, **k):
            r = f(*a, **k)
            self._tape.calls.append((name, r))
            return r
        return call


class _Player:
    """the tape in place of the oracle: the same calls in the same order get the recorded results"""

    def __init__(self, tape):
        self._tape, self._at = tape, 0

    def __getattr__(self, name):
        def call(*a, **k):
            want, r = self._tape.calls[self._at]
            assert want == name, (self._at, want, name)
            self._at += 1
            return r
        return call


class _Oracles:
    """what _pair() takes for the oracle module: Oracle(p, mode) records on first use and replays afterwards"""

    def __init__(self, module, tape):
        self._module, self._tape = module, tape

    def Oracle(self, p, mode="mul"):
        if self._tape.complete:
            return _Player(self._tape)
        self._tape.calls = []
        return _Recorder(self._module.Oracle(p, mode=mode), self._tape)

    def done(self):
        self._tape.complete = True          # (a test that failed half way leaves its tape to be recorded again)


@pytest.fixture(scope="module")
def oracles(O):
    tapes = {}

    def get(kind, perm, which, sequence):
        return _Oracles(O, tapes.setdefault((kind, perm, which, sequence), _Tape()))
    return get


def _fine(s, wide_cells):
    """fine_cell at its default, or the smallest the library takes: a cluster's probe box then spans 8 cells"""
    crp = s.p.collision_range * (1.0 + CS.probe_band(s.p))
    return 2.01 * 1.02 * crp if wide_cells else 0.0


def _hit_pairs(rec):
    pp = rec[rec["j"] >= 0]
    return {(int(min(i, j)), int(max(i, j))) for i, j in zip(pp["i"], pp["j"])}


def _counts_are_the_structure(s, st_sweep):
    """the engine's candidate and cluster counts of the first sweep are the structure's"""
    st = CS.structure(s)
    assert st_sweep["n_candidates"] == len(st["pairs"]), (st_sweep, len(st["pairs"]))
    # n_clusters: the clusters the wide kernel took (isolated pairs and owners, counted per wave into wctl[32 ..]) plus the
    # clusters the ordered workgroup forms in its first round from the candidates left to it (`first && s >= wide_ns &&
    # label[s] == s`, k_resolve); a particle pulled in later has a slot below wide_ns and is not counted.  Together: one per
    # connected component of the candidate graph.
    assert st_sweep["n_clusters"] == len(st["components"]), (st_sweep, len(st["components"]))


def _case_is_real(s, rec):
    """oracle side: the components are what the cases claim, and the pulls and conflicts happen in the sweep's records"""
    st = CS.structure(s)
    comp = st["comp"]
    for case, idx in s.cases.items():
        for q in sorted(set(comp[idx].tolist()) - {-1}):
            c = st["components"][q]
            assert (len(c["particles"]), c["candidates"]) == CS.KNOWN[case], (case, c)
    hits = _hit_pairs(rec)
    roles = s.extra["roles"]

    def hit(a, b):
        return (min(a, b), max(a, b)) in hits

    for r in roles.get("pair_pull1", []) + roles.get("items_over", []) + roles.get("items_fit", []):
        assert comp[r["C"]] == -1 and hit(r["A"], r["B"])
        assert hit(r["A"], r["C"]) == (r["C"] > max(r["A"], r["B"]) or r["B"] < r["C"] < r["A"]), r
    above = [r for r in roles.get("pair_pull1", []) if r["C"] > max(r["A"], r["B"])]
    below = [r for r in roles.get("pair_pull1", []) if r["C"] < min(r["A"], r["B"])]
    if "pair_pull1" in roles:
        assert above and below and all(hit(r["A"], r["C"]) for r in above) and not any(hit(r["A"], r["C"]) for r in below)
    for r in roles.get("pair_pull2", []):
        assert comp[r["C"]] == comp[r["D"]] == -1 and hit(r["A"], r["C"]) and hit(r["B"], r["D"])
    for n in (4, 5):
        for r in roles.get(f"pulls_{n}", []):
            # A's rebound meets the four outsiders around it one after the other.  The fifth of pulls_5, straight behind,
            # is out of A's reach by then: the oracle never hits it, and the kernel's fifth pull is the conservative one of
            # its grid half, which probes where A's FIRST rebound ended
            out = [r[f"O{k}"] for k in range(n)]
            assert all(comp[o] == -1 for o in out) and sum(hit(r["A"], o) for o in out) == 4, (n, r)
            assert all(hit(r["A"], o) for o in out[:4])
    for r in roles.get("pulls_low", []):
        assert r["O0"] < r["A"] < r["O1"] < r["B"] and comp[r["O0"]] == comp[r["O1"]] == -1
        assert hit(r["A"], r["B"]) and not hit(r["A"], r["O0"]) and not hit(r["A"], r["O1"])
    for d in (2, 3, 4):
        for r in roles.get(f"pull_depth_{d}", []):
            line = [r["A"]] + [r[k] for k in "CDEF"[:d]]
            assert all(comp[o] == -1 for o in line[1:]) and all(hit(a, b) for a, b in zip(line, line[1:])), (d, r)
    for r in roles.get("full_pull", []):
        assert comp[r["C"]] == -1 and hit(r["P0"], r["C"])
    for case in ("conflict_overlay", "conflict_grid"):
        if case in roles:
            cross = [r for r in roles[case] if hit(r["B"], r["C"])]
            assert cross and all(comp[r["B"]] != comp[r["C"]] for r in roles[case]), case


# ---------------------------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("which", STATES)
@pytest.mark.parametrize("kind", CS.KINDS)
@pytest.mark.parametrize("perm", CS.PERMS)
@pytest.mark.parametrize("detect_mode", [1, 2])
@pytest.mark.parametrize("wide_cells", [False, True])
def test_every_cluster_case_equals_the_oracle(Engine, oracles, kind, perm, detect_mode, wide_cells, which):
    """one step stage by stage (state after drift, walls and sweep, n_pp, records), then timestep x 2 and run(3) with the
    counters — the plan of amc_timestep and of a short amc_run (wide kernel, then the ordered workgroup in every sweep).
    Then, list-based detection only, amc_run for ON_DEMAND_STEPS steps from the fresh state: the wide kernel alone, and the
    ordered workgroup only after a wave has raised the sticky word (amc_run takes that plan from AMC_OD_MIN_STEPS = 8
    steps on)."""
    s = CS.catalogue(kind, perm, which)
    assert not s.extra["absent"]
    ctx = (kind, perm, detect_mode, wide_cells, which)
    OT = oracles(kind, perm, which, "stages, 1, 1, 3")
    eng, orc = _pair(Engine, OT, s, detect_mode=detect_mode, fine_cell=_fine(s, wide_cells))
    rec = _stagewise(eng, orc, s, ctx, pore=(kind == "pore"))
    assert not (rec["j"] < 0).any()                 # no wall is near a site: what structure() looks at is the drift's
    _case_is_real(s, rec)
    _steps(eng, orc, s, (1, 1, 3), ctx)
    eng.close()
    OT.done()
    if detect_mode != 1:
        return
    # amc_run on the fresh state: its first sweep is the one with the limits in it
    s = CS.catalogue(kind, perm, which)
    OT = oracles(kind, perm, which, "run")
    eng, orc = _pair(Engine, OT, s, detect_mode=detect_mode, fine_cell=_fine(s, wide_cells))
    _steps(eng, orc, s, (ON_DEMAND_STEPS,), (ctx, "run"))
    od = eng.overlap_stats()
    assert od["on_demand_steps"] >= ON_DEMAND_STEPS, (ctx, od)
    if which != "within":
        assert od["stalls"] > 0, (ctx, od)          # a wave raised the sticky word: the ordered workgroup was asked for
    eng.close()
    OT.done()


# ---------------------------------------------------------------------------------------------------------------- branches
def _debug_figures(eng, capfd):
    """the AMC_DEBUG_RESOLVE figures: waves per kind, the three-particle path's counts, the ordered workgroup's launches"""
    capfd.readouterr()
    eng.kernel_times()
    err = capfd.readouterr().err
    waves = {name.strip(): int(nw) for name, nw in re.findall(r"\[amc k_clusters_wide (\S.*?)\s+(\d+) waves, ", err)}
    m3 = re.search(r"\[three-particle path of lane 0\] (\d+) times, (\d+) continued from the pair's hit", err)
    ml = re.search(r"launches (\d+) \(idle hand-over only (\d+)\)", err)
    assert m3 and ml, err
    return waves, (int(m3.group(1)), int(m3.group(2))), (int(ml.group(1)), int(ml.group(2)))


@pytest.mark.parametrize("which", STATES)
@pytest.mark.parametrize("kind", CS.KINDS)
@pytest.mark.parametrize("perm", CS.PERMS)
def test_the_intended_branch_was_taken(Engine, oracles, monkeypatch, capfd, kind, perm, which):
    """The debug instantiation on a fresh context, one sweep: at most 400 candidates and 512 waves, so every candidate is
    lane 0 of its own timed wave and the figures are exact counts."""
    monkeypatch.setenv("AMC_DEBUG_RESOLVE", "1")        # (read at context creation)
    s = CS.catalogue(kind, perm, which)
    ctx = (kind, perm, which)
    OT = oracles(kind, perm, which, "one step")
    eng, orc = _pair(Engine, OT, s, detect_mode=1)
    st = eng.timestep(s.dt)
    rc, so = orc.timestep(s.dt)
    assert rc == 0 and st["n_pp"] == so["n_pp"], (ctx, st, so)
    assert_state_equal(eng.download(), orc.state(), ctx)
    OT.done()
    _counts_are_the_structure(s, st)
    waves, (three, cont), (launches, idle) = _debug_figures(eng, capfd)
    print(ctx, waves, "three-particle path", three, "continued", cont, "launches", launches, "idle", idle)
    want = CS.expected_waves(s)
    for k in KINDS_WAVE:
        assert waves.get(k, 0) + waves.get(k + "+again", 0) == want[k], (ctx, k, waves, want)
    again = {k: waves.get(k + "+again", 0) for k in KINDS_WAVE}
    roles = s.extra["roles"]
    if which == "within":
        # the three bystanders of pair_pull1 are pulled in by pairs; pulls_4, pulls_low and pull_depth_2 pull by 4-clusters
        assert again == {"pair": len(roles["pair_pull1"]), "3-cluster": 0, "4+-cluster": 3, "not owner": 0}, (ctx, again)
    else:
        expect = dict.fromkeys(KINDS_WAVE, 0)
        if which in PULLS_FROM:
            expect[PULLS_FROM[which]] = 1
        assert again == expect, (ctx, again)
    assert (cont, three) == CS.expected_cont(s), (ctx, three, cont)
    assert launches == 1 and idle == (1 if which == "within" else 0), (ctx, launches, idle)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------- one wave
@pytest.mark.parametrize("which", STATES + ("items_over", "items_fit"))
@pytest.mark.parametrize("blocks", [1, 4])
@pytest.mark.parametrize("kind", CS.KINDS)
def test_clusters_sharing_a_wave(Engine, oracles, monkeypatch, capfd, kind, blocks, which):
    """AMC_CW_BLOCKS waves after a warm-up sweep of the same state (the lagging host count then gives up to 64 candidates
    per wave), every catalogue under every permutation: multi-hit clusters emulated in lockstep with their work items
    interleaved; the self edge of the last emulation, the fifth pull's merge edge, the counter-allocated third hit and the
    two conflicting pairs in a wave whose other lanes are live.  A state that crosses a fence still needs the ordered
    workgroup.  items_over: 64 clusters of two hits in one wave and pass bring 256 work items, more than CW_ITEMS — the
    ordered workgroup is needed; 40 clusters fit, and so do 80 over four waves (25 candidates each, 100 items)."""
    monkeypatch.setenv("AMC_CW_BLOCKS", str(blocks))
    monkeypatch.setenv("AMC_DEBUG_RESOLVE", "1")
    seen = []
    for perm in CS.PERMS:
        s = CS.catalogue(kind, perm, which)
        ctx = (kind, perm, which, blocks)
        OT = oracles(kind, perm, which, "1, 1, 2")
        eng, orc = _pair(Engine, OT, s, detect_mode=1)
        eng.timestep(s.dt)                          # warm-up: the host's copy of the candidate count
        a = s.arrays()
        eng.upload(*a[:10], flag=a[10])
        eng.drain_paths()
        _, _, (l0, i0) = _debug_figures(eng, capfd)
        _steps(eng, orc, s, (1,), ctx)              # the sweep with up to 64 candidates per wave
        _, _, (l1, i1) = _debug_figures(eng, capfd)
        seen.append((ctx, "launches, idle before", (l0, i0), "after", (l1, i1)))
        assert l1 - l0 == 1, (ctx, l0, l1)
        if which in CS.HANDOVER or (blocks == 1 and which == "items_over"):
            assert i1 - i0 == 0, (ctx, i0, i1)      # a fence was crossed (items_over: the wave ran out of work items)
        if which == "items_fit" or (blocks == 4 and which == "items_over"):
            assert i1 - i0 == 1, (ctx, i0, i1)      # everything fitted: the ordered workgroup only handed the counters over
        _steps(eng, orc, s, (1, 2), ctx)
        eng.close()
        OT.done()
    print(*seen, sep="\n")


# ---------------------------------------------------------------------------------------------------------------- candidate order
@pytest.mark.parametrize("knob", ["detect_bs", "stream_bs", "list_keep"])
def test_within_limit_clusters_under_other_candidate_orders(Engine, oracles, monkeypatch, knob):
    env, kinds = {"detect_bs": ({"AMC_DETECT_BS": "64"}, CS.KINDS), "stream_bs": ({"AMC_STREAM_BS": "64"}, CS.KINDS),
                  "list_keep": ({"AMC_LIST_KEEP": "3"}, ("pore",))}[knob]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for kind in kinds:
        for perm in CS.PERMS:
            s = CS.catalogue(kind, perm, "within")
            OT = oracles(kind, perm, "within", "1, 3, 1")
            eng, orc = _pair(Engine, OT, s, detect_mode=1)
            _steps(eng, orc, s, (1, 3, 1), (knob, kind, perm))
            eng.close()
            OT.done()


# ---------------------------------------------------------------------------------------------------------------- sharded
SHARDED_STEPS = 3


def _sharded_worker(rank, world, port, q):
    import os

    import torch.distributed as dist
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        try:
            from argon_monte_carlo_amd.dist import ShardedSimulation
            out = {}
            for kind in CS.KINDS:
                for which in STATES:
                    s = CS.catalogue(kind, "identity", which)
                    s.p.detect_mode = 1
                    sim = ShardedSimulation(s.p, rank, world, backend="gloo")
                    a = s.arrays()
                    sim.upload(*a[:10], flag=a[10])
                    tot = sim.run(s.dt, SHARDED_STEPS)
                    out[(kind, which)] = (sim.download(), tot, sim.replicated_detect)
                    sim.engine.close()
            if rank == 0:
                q.put(("ok", out))
        finally:
            dist.destroy_process_group()
    except BaseException as e:
        import traceback
        q.put(("error", f"rank {rank}: {e!r}\n{traceback.format_exc()}"))
        raise


def test_cluster_cases_sharded_by_index_equal_the_oracle(O, monkeypatch):
    """two ranks on one GPU, detection by index: the candidate records and marks the wide kernel decides from are written
    by k_ingest_candidates, not by the detect kernel"""
    from tests.test_gpu_dist import _run_ranks
    monkeypatch.setenv("AMC_MG_REPLICATED", "0")
    out = _run_ranks(2, (), target=_sharded_worker)
    for kind in CS.KINDS:
        for which in STATES:
            s = CS.catalogue(kind, "identity", which)
            s.p.detect_mode = 1
            orc = O.Oracle(s.p, mode="mul")
            a = s.arrays()
            orc.upload(*a[:10], flag=a[10])
            npp = 0
            for _ in range(SHARDED_STEPS):
                rc, so = orc.timestep(s.dt)
                assert rc == 0
                npp += so["n_pp"]
            full, tot, replicated = out[(kind, which)]
            assert not replicated, (kind, which)                # the two-collective form: candidates ingested, not detected
            assert tot["n_pp"] == npp > 0, (kind, which, tot, npp)
            assert_state_equal(full, orc.state(), ("sharded", kind, which))
