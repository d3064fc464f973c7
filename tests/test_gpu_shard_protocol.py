"""GPU (-m gpu): the call order of the sharded step (amc_mg_step, csrc/amc_internal.h; include/argonmc.h, "multi-GPU").

  amc_mg_local -> amc_mg_pack -> all-gather -> amc_mg_sweep -> amc_mg_finish                                      (replicated)
  amc_mg_local -> amc_mg_pack -> all-gather -> amc_mg_detect -> all-gather -> amc_mg_resolve -> amc_mg_finish     (by index)

A call out of place — a step, a run or a stage call of the context's own included — returns AMC_ERR_STATE before it enqueues
anything and leaves the pending step as it was; an entry point that begins a sharded step or replaces the state abandons the
pending step, and the next amc_mg_sweep / amc_mg_detect says so.
Two ShardEngines in one process (dist.LocalRanks: copies on the one stream instead of the collectives) run the phases one at
a time; every comparison is with the oracle (`orc_mul`) stepped on the CPU, bit for bit: no tolerances.

The systems are test_gpu_dist._tiny_case("cube" | "pore", 257) over TINY_STEPS = 7 steps: rank 0 owns 129 particles, rank 1
owns 128; the grid detector works at any size (detect_mode = 1) and the pore's kept lists (K = 4: full builds at steps 0 and
4) cross a full rebuild.  Non-vacuity, asserted on the oracle's own output before any cell runs (`reference`): every sweep has
at least 18 p-p collisions and at least 10 particles of each rank's range change velocity bitwise in every step — a lost
velocity list or a sweep resolved twice changes the state at any step.
"""
import numpy as np
import pytest
import torch                # (first: the library then shares torch's HIP runtime — the ranks exchange through torch)

from argon_monte_carlo_amd._abi import AMC_ERR_STATE
from argon_monte_carlo_amd._lib import ArgonMCError
from argon_monte_carlo_amd.dist import LocalRanks, shard_range
from tests.test_gpu_dist import TINY_STEPS, _tiny_case

pytestmark = pytest.mark.gpu

N, WORLD = 257, 2
RANGES = [shard_range(N, r, WORLD) for r in range(WORLD)]
KINDS = ("cube", "pore")
KEYS = ["x", "y", "z", "vx", "vy", "vz", "d", "dx", "dy", "dz", "flag"]
MIN_PP, MIN_CHANGED = 18, 10


def build_reference():
    """kind -> (params, dt, init, the oracle's state at the start, its (state, counters) after every step, a single Engine's
    histograms)."""
    from argon_monte_carlo_amd.engine import Engine
    from oracle import oracle
    ref = {}
    for kind in KINDS:
        p, dt, init = _tiny_case(kind, N)
        orc = oracle.Oracle(p, mode="mul")
        orc.upload(*init)
        start = orc.state()
        steps, prev = [], start
        for s in range(TINY_STEPS):
            rc, so = orc.timestep(dt)
            assert rc == 0, (kind, s)
            st = orc.state()
            changed = (st["vx"] != prev["vx"]) | (st["vy"] != prev["vy"]) | (st["vz"] != prev["vz"])
            assert so["n_pp"] >= MIN_PP, (kind, s, so)
            for lo, hi in RANGES:
                assert np.count_nonzero(changed[lo:hi]) >= MIN_CHANGED, (kind, s, lo, hi)
            steps.append((st, so))
            prev = st
        eng = Engine(p)
        try:
            eng.upload(*init)
            eng.run(dt, TINY_STEPS)
            counts, tot = eng.histograms()
        finally:
            eng.close()
        ref[kind] = (p, dt, init, start, steps, (counts.astype(np.int64), int(tot)))
    return ref


@pytest.fixture(scope="module")
def reference():
    return build_reference()


class Job:
    """Two ranks on one system, stepped phase by phase."""
    REPLICATED = ("local", "pack", "exchange", "sweep", "finish")
    BY_INDEX = ("local", "pack", "exchange", "detect", "exchange_candidates", "resolve", "finish")

    def __init__(self, ref, kind, replicated, candidates=False):
        from argon_monte_carlo_amd.engine import ShardEngine
        self.kind, self.replicated = kind, replicated
        self.p, self.dt, self.init, self.start, self.steps, self.hist = ref[kind]
        stream = torch.cuda.current_stream().cuda_stream
        self.engs = [ShardEngine(self.p, lo, hi) for lo, hi in RANGES]
        for e in self.engs:
            e.set_stream(stream)                # (the exchange is torch's: same stream)
            e.upload(*self.init)
        self.ranks = LocalRanks(self.engs, replicated=replicated)
        if candidates:                          # (the replicated form with the candidate blocks in place: amc_mg_resolve could run)
            for e in self.engs:
                e.candidate_buffers(WORLD)

    def close(self):
        for e in self.engs:
            e.close()

    def restart(self):
        """the whole initial state on both ranks (path accumulators and flags too)"""
        for e in self.engs:
            e.upload(*[self.start[k] for k in KEYS[:10]], flag=self.start["flag"])
            e.reset_outputs()       # (the counters are deltas between two reads: what the abandoned step counted goes)

    def phase(self, name):
        R = self.ranks
        if name == "local":
            R.local(self.dt)
        elif name == "exchange_candidates":
            R.exchange(candidates=True)
        elif name == "finish":
            return R.finish(True)
        else:
            getattr(R, name)()

    def step(self, after=None, intruder=None):
        """one step in the legal order; `intruder` runs directly behind the phase `after`.  Returns n_pp (rank 0's) and the
        summed n_paths."""
        for name in (self.REPLICATED if self.replicated else self.BY_INDEX):
            sts = self.phase(name)
            if name == after:
                intruder()
        return {"n_pp": sts[0]["n_pp"], "n_paths": sum(s["n_paths"] for s in sts)}

    def assert_step(self, s, st, what):
        """the owners' ranges of the state and the step's counters against the oracle's step `s`"""
        ref_state, so = self.steps[s]
        parts = [e.download() for e in self.engs]
        state = {k: np.concatenate([d[k][lo:hi] for d, (lo, hi) in zip(parts, RANGES)]) for k in KEYS}
        for k in KEYS:
            got, want = (state[k].astype(bool), ref_state[k].astype(bool)) if k == "flag" else (state[k], ref_state[k])
            assert np.array_equal(got, want), (what, self.kind, self.replicated, s, k, np.flatnonzero(got != want)[:5])
        if st is not None:
            for k in ("n_pp", "n_paths"):
                assert st[k] == so[k], (what, self.kind, self.replicated, s, k, st, so)

    def assert_histograms(self, what):
        res = [e.histograms() for e in self.engs]
        counts, tot = sum(r[0].astype(np.int64) for r in res), sum(int(r[1]) for r in res)
        assert tot == self.hist[1] and np.array_equal(counts, self.hist[0]), (what, self.kind, tot, self.hist[1])


@pytest.fixture
def job(reference):
    made = []

    def make(kind, replicated, **kw):
        made.append(Job(reference, kind, replicated, **kw))
        return made[-1]
    yield make
    for j in made:
        j.close()


def refused(call, *args):
    """`call` must fail with AMC_ERR_STATE; returns the message"""
    with pytest.raises(ArgonMCError) as err:
        call(*args)
    assert err.value.code == AMC_ERR_STATE, err.value
    print("refused:", err.value)
    return str(err.value)


# ---------------------------------------------------------------------------------------------- a. control
@pytest.mark.parametrize("replicated", [True, False], ids=["replicated", "by_index"])
@pytest.mark.parametrize("kind", KINDS)
def test_control_seven_steps_equal_oracle(job, kind, replicated):
    j = job(kind, replicated)
    for s in range(TINY_STEPS):
        j.assert_step(s, j.step(), "control")
    j.assert_histograms("control")


# ---------------------------------------------------------------------------------------------- b. refusals that leave the step intact
def _bounds(e):
    e._ck(e.lib.amc_mg_bounds(e._ctx))


# name -> (replicated form, candidate blocks in place, the phase it follows, the misplaced call on rank 0's engine)
MISPLACED = {
    "second_pack": (True, False, "pack", lambda e: e.mg_pack(WORLD)),
    "resolve_before_detect": (False, False, "exchange", lambda e: e.mg_resolve(WORLD)),
    "detect_twice": (False, False, "detect", lambda e: e.mg_detect(WORLD, 0)),
    "sweep_after_detect": (False, False, "detect", lambda e: e.mg_sweep(WORLD, 0)),
    "resolve_after_sweep": (True, True, "sweep", lambda e: e.mg_resolve(WORLD)),
    "finish_before_sweep": (True, False, "exchange", lambda e: e.mg_finish(True)),
    "bounds_after_pack": (True, False, "pack", _bounds),
    # a step, a run or a sweep of the context's own in the middle of the ranks' step
    "own_timestep_after_pack": (True, False, "pack", lambda e: e.timestep(1e-14)),
    "own_run_after_exchange": (True, False, "exchange", lambda e: e.run(1e-14, 2)),
    "own_stage_sweep_after_detect": (False, False, "detect", lambda e: e.stage_sweep()),
}


@pytest.mark.parametrize("at", [1, 4], ids=["step_in_between", "full_rebuild"])      # (of the pore's kept-list cycle)
@pytest.mark.parametrize("name", list(MISPLACED))
@pytest.mark.parametrize("kind", KINDS)
def test_misplaced_call_is_refused_and_the_step_completes(job, kind, name, at):
    replicated, candidates, after, call = MISPLACED[name]
    j = job(kind, replicated, candidates=candidates)
    for s in range(TINY_STEPS):
        if s == at:
            st = j.step(after, lambda: refused(call, j.engs[0]))
        else:
            st = j.step()
        j.assert_step(s, st, name)
    j.assert_histograms(name)


# ---------------------------------------------------------------------------------------------- c. intruders that invalidate a pack
def _set_shard(e):
    e._ck(e.lib.amc_set_shard(e._ctx, e.lo, e.hi))


# (amc_timestep, amc_run and the stage calls are no intruders of this kind: in the middle of a sharded step they are refused
# themselves, the cells "own_*" of MISPLACED above.)
INTRUDERS = {
    "mg_local": lambda e, j: e.mg_local(j.dt),
    "upload": lambda e, j: e.upload(*j.init),
    "set_shard": lambda e, j: _set_shard(e),
    "other_world": lambda e, j: e.exchange_buffers(3),
}


@pytest.mark.parametrize("replicated", [True, False], ids=["replicated", "by_index"])
@pytest.mark.parametrize("name", list(INTRUDERS))
@pytest.mark.parametrize("kind", KINDS)
def test_intruder_invalidates_the_pack_and_leaves_nothing_behind(job, kind, name, replicated):
    j = job(kind, replicated)
    j.assert_step(0, j.step(), "before the intruder")
    j.phase("local")
    j.phase("pack")
    e = j.engs[0]
    INTRUDERS[name](e, j)
    assert "without amc_mg_pack in this step" in refused(e.mg_sweep, WORLD, 0)
    if not replicated:
        refused(e.mg_detect, WORLD, 0)
    # recovery: the views of this world size again where it was changed, the initial state on both ranks, two steps
    j.ranks.buffers()
    j.restart()
    for s in range(2):
        st = j.step()
        j.assert_step(s, st, name)
